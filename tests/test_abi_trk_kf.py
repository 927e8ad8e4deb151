"""C-ABI checks of the Kalman tracking loop's entry points that need no GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np

import gsdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsdr.h")
NEW = ("gsdr_trk_kf_conf_default", "gsdr_trk_set_kf", "gsdr_trk_get_kf_state")
DEFAULTS = (0.2, 0.3, 0.15, 0.25, 0.6, 0.01, 0.5, 0.7, 5.0, 1.0)


def test_header_declares_the_kalman_entry_points():
    txt = open(HEADER).read()
    assert re.search(r"typedef struct gsdr_trk_kf_conf\s*\{[^}]*\}\s*gsdr_trk_kf_conf;", txt)
    assert re.search(r"void gsdr_trk_kf_conf_default\(gsdr_trk_kf_conf\* conf\);", txt)
    assert re.search(r"int gsdr_trk_set_kf\(gsdr_trk\* trk, const gsdr_trk_kf_conf\* conf\);", txt)
    assert re.search(r"int gsdr_trk_get_kf_state\(gsdr_trk\* trk, int ch, double x\[4\], double P\[16\]\);", txt)
    L = gsdr.load()
    for name in NEW:
        assert name in gsdr.EXPORTED and hasattr(L, name), name
    for name in ("KF_CONF_DTYPE", "trk_kf_conf_default"):
        assert hasattr(gsdr, name), name
    assert hasattr(gsdr.Tracking, "set_kf") and hasattr(gsdr.Tracking, "kf_state")


def test_kf_conf_layout_matches_c_compiler(tmp_path):
    dt = gsdr.KF_CONF_DTYPE
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsdr.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(gsdr_trk_kf_conf));']
    for f in dt.names:
        lines.append('printf("%s %%zu\\n", offsetof(gsdr_trk_kf_conf, %s));' % (f, f))
    lines.append("return 0;}")
    src, exe = tmp_path / "kf_layout.c", tmp_path / "kf_layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == dt.itemsize == 80
    assert len(dt.names) == 10
    for f in dt.names:
        assert int(got[f]) == dt.fields[f][1], f


def test_kf_conf_defaults():
    c = gsdr.trk_kf_conf_default()
    assert c.dtype == gsdr.KF_CONF_DTYPE and len(c) == 1
    assert tuple(float(c[f][0]) for f in gsdr.KF_CONF_DTYPE.names) == DEFAULTS
    gsdr.load().gsdr_trk_kf_conf_default(None)  # a null pointer is ignored


def test_existing_abi_is_unchanged():
    assert gsdr.load().gsdr_abi_version() == 1
    assert gsdr.TRK_CONF_DTYPE.itemsize == 144


def test_null_handle_is_rejected():
    L = gsdr.load()
    c = gsdr.trk_kf_conf_default()
    x, P = np.zeros(4), np.zeros(16)
    assert L.gsdr_trk_set_kf(None, ctypes.c_void_p(c.ctypes.data)) == gsdr.GSDR_E_ARG
    assert b"null" in L.gsdr_last_error()
    assert L.gsdr_trk_get_kf_state(None, 0, ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(P.ctypes.data)) == gsdr.GSDR_E_ARG
    assert b"null" in L.gsdr_last_error()
    assert not x.any() and not P.any()
