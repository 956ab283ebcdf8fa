"""Sliced Arrow record batches for the two consumers of an incoming Arrow C array: the IPC file writer (tests/test_ipc.py, CPU)
and the device importer (tests/test_types_gpu.py).  Both take an array's `offset` out of every buffer through the same
normaliser, so both tests run the same slices: start offsets and lengths around the byte (8) and bitmap word (64) boundaries,
where a bitmap has to be re-aligned bit by bit, plus one length of many words."""
import functools

import numpy as np

STARTS = [0, 1, 7, 8, 9, 63, 64, 65]
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 1000]
ROWS = max(STARTS) + max(LENGTHS)


@functools.lru_cache(maxsize=None)
def _base():
    import pyarrow as pa
    rng = np.random.default_rng(17)
    n = ROWS

    def maybe(vals, p=0.2):
        return [None if rng.random() < p else v for v in vals]

    words = ["", "a", "é日本", "gamma-gamma", "", "xy"]
    text = [words[k] + (str(i) if k > 1 else "") for i, k in enumerate(rng.integers(0, len(words), n))]
    return pa.record_batch({
        "i32": pa.array(maybe(rng.integers(-2 ** 31, 2 ** 31 - 1, n).tolist()), pa.int32()),
        "b": pa.array(maybe((rng.random(n) > 0.5).tolist()), pa.bool_()),
        "s": pa.array(maybe(text), pa.string()),
        "ls": pa.array(maybe(text[::-1], 0.1), pa.large_string()),
        "bin": pa.array(maybe([t.encode()[::-1] for t in text], 0.1), pa.binary()),
    })


def sliced(start, length):
    """rows [start, start + length) of the base batch as a slice (nothing copied: every array carries the offset), and a NULL-free
    Int64 column whose array still brings a validity buffer, all ones, with its null count left unknown"""
    import pyarrow as pa
    sl = _base().slice(start, length)
    ones = pa.py_buffer(b"\xff" * ((ROWS + 7) // 8))
    values = pa.py_buffer((np.arange(ROWS, dtype=np.int64) * 3 - 7).tobytes())
    all_valid = pa.Array.from_buffers(pa.int64(), length, [ones, values], null_count=-1, offset=start)
    return pa.record_batch(sl.columns + [all_valid], names=sl.schema.names + ["all_valid"])
