"""The tracking ABI of the 10.23 Mcps signals: GSDR_SIGNAL_GAL_5X / GSDR_SIGNAL_GPS_L5 and
gsdr_trk_set_secondary_code.  The declaration checks need no GPU; gsdr_trk_create opens a
device, so everything that takes a handle is marked gpu."""
import os
import re

import numpy as np
import pytest

import gsdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wideband_tracking_is_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "gsdr.h")).read()
    assert re.search(r"#define\s+GSDR_SIGNAL_GAL_5X\s+3\b", txt) and re.search(r"#define\s+GSDR_SIGNAL_GPS_L5\s+4\b", txt)
    assert (gsdr.SIGNAL_GAL_5X, gsdr.SIGNAL_GPS_L5) == (3, 4)
    assert "gsdr_trk_set_secondary_code" in set(re.findall(r"\b(gsdr_[a-z0-9_]+)\s*\(", txt))
    assert "gsdr_trk_set_secondary_code" in gsdr.EXPORTED
    L = gsdr.load()
    assert L.gsdr_abi_version() == 1  # an entry point and two constants were added; no layout changed
    assert gsdr.TRK_CONF_DTYPE.itemsize == 144
    assert L.gsdr_trk_set_secondary_code(None, 0, b"01", 2) == gsdr.GSDR_E_ARG


def _conf(signal, pilot=1):
    c = gsdr.trk_conf_default()
    c["fs_in"] = 4.0e6
    c["signal"] = signal
    c["track_pilot"] = pilot
    return c


def _code(t, ch, bits, n=None):
    b = bits.encode()
    return gsdr.load().gsdr_trk_set_secondary_code(t._h, ch, b, len(b) if n is None else n)


@pytest.mark.gpu
def test_create_takes_signals_3_and_4_and_refuses_5():
    for sig in (gsdr.SIGNAL_GAL_5X, gsdr.SIGNAL_GPS_L5):
        for pilot in (1, 0):
            gsdr.Tracking(_conf(sig, pilot)).close()
    with pytest.raises(gsdr.GsdrError) as e:
        gsdr.Tracking(_conf(5))
    assert e.value.code == gsdr.GSDR_E_UNSUPPORTED


@pytest.mark.gpu
def test_e5a_pilot_start_needs_the_secondary_code():
    code = np.ones(10230, np.float32)
    t = gsdr.Tracking(_conf(gsdr.SIGNAL_GAL_5X, 1))
    with pytest.raises(gsdr.GsdrError) as e:
        t.start(0, 11, code, 100.0, 0.0, 0, 0, data_code=code)
    assert e.value.code == gsdr.GSDR_E_STATE
    assert _code(t, 0, "01" * 50) == gsdr.GSDR_OK
    assert t.start(0, 11, code, 100.0, 0.0, 0, 0, data_code=code) == 4100
    t.close()
    # data tracking, and L5 in both modes, start without one
    for sig, pilot in ((gsdr.SIGNAL_GAL_5X, 0), (gsdr.SIGNAL_GPS_L5, 1), (gsdr.SIGNAL_GPS_L5, 0)):
        t = gsdr.Tracking(_conf(sig, pilot))
        assert t.start(0, 11, code, 100.0, 0.0, 0, 0, data_code=code if pilot else None) == 4100
        t.close()


@pytest.mark.gpu
def test_set_secondary_code_refusals():
    t = gsdr.Tracking(_conf(gsdr.SIGNAL_GAL_5X, 1))
    assert _code(t, 0, "0" * 161, 0) != gsdr.GSDR_OK
    assert _code(t, 0, "0" * 161, 161) != gsdr.GSDR_OK
    assert _code(t, 0, "0" * 160, 160) == gsdr.GSDR_OK and _code(t, 0, "1", 1) == gsdr.GSDR_OK
    assert _code(t, 0, "01x1") == gsdr.GSDR_E_ARG
    assert _code(t, 1, "01") == gsdr.GSDR_E_ARG  # max_channels is 1
    t.close()
    for sig, pilot in ((gsdr.SIGNAL_GPS_1C, 1), (gsdr.SIGNAL_GAL_1B, 1), (gsdr.SIGNAL_BDS_B1, 1), (gsdr.SIGNAL_GAL_5X, 0),
                       (gsdr.SIGNAL_GPS_L5, 1), (gsdr.SIGNAL_GPS_L5, 0)):
        t = gsdr.Tracking(_conf(sig, pilot))
        assert _code(t, 0, "01" * 10) == gsdr.GSDR_E_STATE, (sig, pilot)
        t.close()
