"""The host-side rules of bringing caller rows from host memory (ligero-prover_amd/csrc/upload_plan.hpp: the uploader thread's pick
order, presence masks as copy / zero-fill runs, the jobs of a chunk schedule, the flag words of a trace and of a shard) as a
stand-alone host program under AddressSanitizer and UBSan: no GPU, no library, nothing loaded into python.  What it checks is
written out in tests/cpp/upload_plan_prog.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "upload_plan_prog.cpp")


def test_upload_plan_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "upload_plan_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert out.strip().splitlines()[-1] == "upload plan ok", out
