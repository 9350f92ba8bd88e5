"""The staging layout of the host entry points (openkite_amd/csrc/stage_layout.hpp)
without a device: tests/stage_layout_check.cpp is built against the header with
the address and undefined-behaviour sanitizers and run.  It checks the offsets
and totals of kite_nmpc_windekf_step (count 1 and 5, with and without z, with
and without a status pointer), kite_nmpc_plant_step_delayed without a command
and kite_nmpc_score_step with one of its int32 inputs missing against values
written out by hand, that every segment starts 8-byte aligned, that none
overlap and that an odd int32 count rounds up."""
import os
import shutil
import subprocess


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_layout_program(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ (the compiler the library's driver is built with) is needed"
    exe = str(tmp_path / "stage_layout_check")
    subprocess.run([gxx, "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "openkite_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "stage_layout_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"
