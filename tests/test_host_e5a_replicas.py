"""The Galileo E5a replica generator of the host adapters (gnss-sdr-new_amd/host/gnss_replicas.cc:
galileo_e5a_load_code_table, galileo_e5_a_code_gen_complex_sampled) against the restatement of
galileo_e5_signal_replica.cc:31-124 in tests/iq_caf_checks.py, bit-exact, on a seeded random code
table written to a temporary directory (the repository ships none).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import iq_caf_checks as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "gnss-sdr-new_amd", "build", "replica_dump")


def dump(kind, prn, fs, shift, table):
    assert os.path.exists(TOOL), "replica_dump not built (python __graft_entry__.py)"
    r = subprocess.run([TOOL, kind, str(prn), str(fs), str(shift), str(table)], capture_output=True)
    return r.returncode, np.frombuffer(r.stdout, np.float32).view(np.complex64), r.stderr.decode()


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    data = qc.e5a_random_table(4242)
    assert len(data) == 100 * qc.E5A_ROW_BYTES
    path = tmp_path_factory.mktemp("e5a") / "codes.bin"
    path.write_bytes(data)
    return data, path


@pytest.mark.parametrize("prn", [1, 23, 50])
def test_sampled_codes(table, prn):
    data, path = table
    for fs in (4000000, 10230000, 32000000):
        for kind, signal in (("e5a_i", "5I"), ("e5a_q", "5Q"), ("e5a_x", "5X")):
            for shift in (0, 1, 5000):
                rc, got, _ = dump(kind, prn, fs, shift, path)
                assert rc == 0
                np.testing.assert_array_equal(got, qc.e5a_sampled(data, prn, signal, fs, shift))
    # 5I and 5Q are real-valued rows of +-1, 5X is I + jQ of the same chips
    i, q, x = (dump(k, prn, 10230000, 0, path)[1] for k in ("e5a_i", "e5a_q", "e5a_x"))
    assert not i.imag.any() and not q.imag.any() and set(np.unique(i.real)) == {-1.0, 1.0}
    np.testing.assert_array_equal(x, i.real + 1j * q.real)
    # the layout: MSB first, a set bit is -1; PRN p of E5a-Q is row 50 + p - 1
    rows = np.frombuffer(data, np.uint8).reshape(100, qc.E5A_ROW_BYTES)
    assert i.real[0] == (-1.0 if rows[prn - 1, 0] & 0x80 else 1.0)
    assert q.real[9] == (-1.0 if rows[50 + prn - 1, 1] & 0x40 else 1.0)


def test_refusals(table, tmp_path):
    data, path = table
    rc, _, err = dump("e5a_i", 1, 4000000, 0, tmp_path / "absent.bin")
    assert rc == 3 and "cannot be read" in err
    short = tmp_path / "short.bin"
    short.write_bytes(data[:-1])
    rc, _, err = dump("e5a_i", 1, 4000000, 0, short)
    assert rc == 3 and "127899 bytes" in err and "127900" in err
    for prn in (0, 51):
        assert dump("e5a_x", prn, 4000000, 0, path)[0] == 4
