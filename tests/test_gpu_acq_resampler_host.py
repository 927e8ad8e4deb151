"""GNSS-SDR.use_acquisition_resampler on the host mirror's device-ring path
(gnss-sdr-new_amd/host/acq_resampler.*, AcquisitionService::attach_resampler,
gsdr_factory::GetAcqService): host/tests/resampler_selftest.cc on the GPU -- the
hub hands two services of one (device, ring key, signal) the same decimator, and a
service with the resampler attached acquires synthetic GPS at 16 Msps on the
2 Msps decimated ring with its answers mapped back to the input rate
(pcps_acquisition.cc:699-705)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnss-sdr-new_amd", "host")
BUILD = os.path.join(ROOT, "gnss-sdr-new_amd", "build")


@pytest.mark.gpu
def test_resampler_selftest_on_gpu():
    exe = os.path.join(BUILD, "resampler_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "resampler_selftest: PASS" in r.stdout
