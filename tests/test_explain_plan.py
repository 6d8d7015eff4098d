"""The host-side rules of lig_rows_explain (ligero-prover_amd/csrc/explain_plan.hpp: which asked lists and slots are accepted, the order of
the term records, where every constraint's records begin) as a stand-alone host program under AddressSanitizer and UBSan: no GPU, no
library, nothing loaded into python.  What it checks is written out in tests/cpp/explain_plan_prog.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "explain_plan_prog.cpp")


def test_explain_plan_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "explain_plan_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert out.strip().splitlines()[-1] == "explain plan ok", out
