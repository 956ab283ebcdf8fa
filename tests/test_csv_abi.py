"""CPU tier of the CSV scan: include/ballista_hip.h declares bhip_batch_from_csv and its options struct, the library exports
it, the ctypes binding mirrors it, and arguments are checked before any device is touched."""
import ctypes as C
import os
import re

import ballista_amd as ba
from ballista_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_from_csv():
    text = open(os.path.join(ROOT, "include", "ballista_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"bhip_status\s+bhip_batch_from_csv\s*\(([^)]*)\)", code)
    assert m, "bhip_batch_from_csv is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 9 and "bhip_csv_opts" in params[7] and params[8].startswith("bhip_batch**")
    s = re.search(r"typedef struct bhip_csv_opts\s*\{([^}]*)\}\s*bhip_csv_opts;", code)
    assert s, "bhip_csv_opts is not declared"
    members = [re.split(r"\s+", d.strip()) for d in s.group(1).split(";") if d.strip()]
    assert members == [["uint8_t", "delimiter"], ["int32_t", "has_header"]]
    assert [(n, t) for n, t in L.CsvOpts._fields_] == [("delimiter", C.c_uint8), ("has_header", C.c_int32)]
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "bhip_batch_from_csv")
    res, args = L.SYMBOLS["bhip_batch_from_csv"]
    assert res is C.c_int32 and len(args) == 9


def test_null_arguments_are_reported_not_dereferenced():
    lib = L.lib()
    h = C.c_void_p()
    assert lib.bhip_batch_from_csv(None, None, 0, 0, None, 0, None, None, C.byref(h)) == L.EINVAL
    assert b"null" in lib.bhip_last_error()
    assert hasattr(ba.RecordBatch, "from_csv")
