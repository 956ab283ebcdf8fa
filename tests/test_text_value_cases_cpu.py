"""The case table of the text scans' value grammar (tests/text_value_cases.py) against Python alone: every accepted string is in
the grammar and converts, every refused one is refused by Python or lies outside the grammar, and the two things the scans accept
that Python does not (text scan: a lone '.', a day its month does not have) are not in it."""
import pytest

import text_value_cases as T


@pytest.mark.parametrize("dtype,s", T.accepted_cases())
def test_accepted_strings_convert(dtype, s):
    assert T.GRAMMAR[dtype].fullmatch(s)
    T.expected(dtype, s)                                   # raises if Python refuses it
    assert dtype != "Float64" or T.exactly_convertible(s)
    assert T.GRAMMAR[dtype].fullmatch(T.PLAIN[dtype])


@pytest.mark.parametrize("dtype,s,error", T.refused_cases())
def test_refused_strings_are_refused(dtype, s, error):
    in_grammar = T.GRAMMAR[dtype].fullmatch(s) is not None
    if error == "NotImplementedOnGpu":                      # a decimal of the grammar, outside the exact conversion
        assert dtype == "Float64" and in_grammar and not T.exactly_convertible(s)
        return
    try:
        T.expected(dtype, s)
        python_refuses = False
    except ValueError:
        python_refuses = True
    assert python_refuses or not in_grammar


def test_known_gaps_are_not_in_the_table():
    strings = [s for _, s in T.accepted_cases()] + [s for _, s, _ in T.refused_cases()]
    assert "." not in strings
    for dtype, s, _ in T.refused_cases():
        if dtype == "Date32" and T.GRAMMAR[dtype].fullmatch(s):
            y, m, d = (int(x) for x in s.split("-"))
            assert not (1 <= m <= 12 and 1 <= d <= 31), s  # refused for a month or day no calendar has, not for an impossible day
