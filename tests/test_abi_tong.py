"""gsdr_acq_tong_result: the ctypes and numpy mirrors against the C compiler's sizeof/offsetof, and
the state constants.  No GPU."""
import ctypes
import os
import re
import subprocess

import gsdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tong_record_layout_matches_c_compiler(tmp_path):
    src = tmp_path / "tong_layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsdr.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(gsdr_acq_tong_result));']
    for f, _ in gsdr.AcqTongResult._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(gsdr_acq_tong_result, %s));' % (f, f))
    for c in ("RUNNING", "POSITIVE", "NEGATIVE", "PAST_END"):
        lines.append('printf("%s %%d\\n", GSDR_TONG_%s);' % (c, c))
    lines.append("return 0;}")
    src.write_text("\n".join(lines))
    exe = tmp_path / "tong_layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    dt = gsdr.ACQ_TONG_RESULT_DTYPE
    assert int(got["size"]) == ctypes.sizeof(gsdr.AcqTongResult) == dt.itemsize == 56
    assert [f for f, _ in gsdr.AcqTongResult._fields_] == list(dt.names)
    for f, _ in gsdr.AcqTongResult._fields_:
        assert int(got[f]) == getattr(gsdr.AcqTongResult, f).offset == dt.fields[f][1], f
    assert (int(got["RUNNING"]), int(got["POSITIVE"]), int(got["NEGATIVE"]), int(got["PAST_END"])) == \
        (gsdr.TONG_RUNNING, gsdr.TONG_POSITIVE, gsdr.TONG_NEGATIVE, gsdr.TONG_PAST_END) == (0, 1, 2, 3)


def test_tong_entry_points_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "gsdr.h")).read()
    names = {"gsdr_acq_set_tong", "gsdr_acq_tong_reset", "gsdr_acq_run_tong", "gsdr_acq_run_tong_stream",
             "gsdr_acq_dump_tong_grid"}
    assert names <= set(re.findall(r"\b(gsdr_[a-z0-9_]+)\s*\(", txt))
    assert names <= set(gsdr.EXPORTED)
    L = gsdr.load()
    assert L.gsdr_abi_version() == 1  # entry points were added; no layout or signature changed
    assert L.gsdr_acq_set_tong(None, 1, 2, 3) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_tong_reset(None, None, 0) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_tong(None, None, 1, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_dump_tong_grid(None, 0, None) == gsdr.GSDR_E_ARG
