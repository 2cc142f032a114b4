"""Runs the native suite of the coin selection's batched subset search (csrc/test/
coinselect_tests.cpp) through bin/test_bcp: the host twin against a bitmap-keeping rewrite of the
reference loop fed the same bits, and SelectCoinsMinConf's contract on lists at or above
-gpucoinselectthreshold."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "test_bcp")


def test_coinselect_native_suite(tmp_path):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", ROOT, "-j8", "unittest"])
    listed = subprocess.run([BIN, "--list"], capture_output=True, text=True, check=True).stdout
    assert "coinselect_tests" in [l.split()[0] for l in listed.splitlines() if l.strip()]
    p = subprocess.run([BIN, "--suite=coinselect_tests"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "4 cases, 0 failed" in p.stdout


def test_option_is_documented():
    bcpd = os.path.join(ROOT, "bin", "bcpd")
    if not os.path.exists(bcpd):
        subprocess.check_call(["make", "-C", ROOT, "-j8", "tools"])
    text = subprocess.run([bcpd, "-help"], capture_output=True, text=True, timeout=60)
    assert "-gpucoinselectthreshold=<n>" in text.stdout + text.stderr
