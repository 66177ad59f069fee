"""CPU check of the IMU factor's block-selecting form (be_factor_dev.h imu_raw_sel, which be_eval's IMU workgroup calls with a share of the blocks per wave):
tests/host/imu_blocks_test.cpp compiles the header for the host with the kernels' floating-point rule (no contraction) and calls the form once per block — the
residual and the 15 x 30 Jacobian must be imu_raw's bit for bit, over eight random factors and one with zero biases, and every call must write its own block only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blocks_reproduce_the_whole_jacobian(tmp_path):
    exe = str(tmp_path / "imu_blocks_test")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function", "-I" + os.path.join(ROOT, "dynamic_vins_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "imu_blocks_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 9", r.stdout + r.stderr
