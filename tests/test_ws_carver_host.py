"""The workspace carver (csrc/frcnn_host.h: WsCarver) on its own: tests/ws_carver_check.cpp is a stand-alone host program that includes
only that header and checks the carver against arithmetic written out by hand -- null base and real base give one total, every piece
256-byte aligned and clear of the next, the any-base mode at base offsets 0, 1, 64 and 255 (first piece at the next boundary, last piece
inside base + bytes(), bytes() = 256 + the plain total), pieces of 0 and 1 byte, and the VOC evaluator's and the detection
post-process's layouts as formulas.  This test compiles it for the host and runs it; no GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ws_carver_check_program(tmp_path):
    exe = str(tmp_path / "ws_carver_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "faster_rcnn_pytorch_amd", "csrc"), os.path.join(ROOT, "tests", "ws_carver_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "checks OK" in r.stdout, r.stdout + r.stderr
