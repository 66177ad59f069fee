"""The line tracker's boundary (CPU): include/dvins.h declares dv_line_track_* and dv_line_match, the library exports them, the ctypes mirror has them with the
header's argument counts, and the struct layouts and limits the Python side mirrors agree with the header."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvins.h")
LIB = os.path.join(ROOT, "dynamic_vins_amd", "lib", "libdvins_hip.so")
ENTRIES = {"dv_line_track_check": 7, "dv_line_track_reset": 1, "dv_line_track_enqueue": 8, "dv_line_track_collect": 11, "dv_line_match": 7}


def header_text():
    src = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_library_and_mirror_have_the_entries():
    from dynamic_vins_amd import _abi
    src = header_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    lib = _abi.load()
    for name, nargs in ENTRIES.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", src, flags=re.M)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == nargs
        assert re.search(r"\b" + name + r"\b", exported), f"{name} is not exported"
        res, args = _abi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib, name).argtypes == args


def test_struct_layouts_and_limits():
    from dynamic_vins_amd import backend, frontend
    src = header_text()
    assert int(re.search(r"#define\s+DV_LINE_MAX\s+(\d+)", src).group(1)) == frontend.DV_LINE_MAX == 512
    assert int(re.search(r"#define\s+DV_LINE_DESC_BYTES\s+(\d+)", src).group(1)) == frontend.DV_LINE_DESC_BYTES == 32
    m = re.search(r"typedef struct dv_key_line \{([^}]*)\}", src)
    assert [f.strip() for f in m.group(1).replace("float", "").strip(" ;").split(",")] == list(frontend.KEYLINE_DTYPE.names)
    assert frontend.KEYLINE_DTYPE.itemsize == 24 and all(frontend.KEYLINE_DTYPE[n].itemsize == 4 for n in frontend.KEYLINE_DTYPE.names)
    assert backend.LINEROW_DTYPE.itemsize == 72 and backend.LINEROW_DTYPE.fields["left"][1] == 8 and backend.LINEROW_DTYPE.fields["right"][1] == 40
