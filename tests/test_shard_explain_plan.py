"""The host-only pieces of lig_shard_rows_explain / lig_shard_rows_read_slots (ligero-prover_amd/csrc/explain_plan.hpp: the items of the
asked constraints from a term list, the piece schedule of the value exchange) as a stand-alone host program under AddressSanitizer and
UBSan: no GPU, no library, nothing loaded into python.  What it checks is written out in tests/cpp/shard_explain_plan_prog.cpp; the
order of the items it prints is restated here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shard_explain_plan_prog.cpp")
ONE, NEG_ONE = 0xFFFFFFFF, 0xFFFFFFFE

# the system of the program: constraint -> its (slot, coefficient index) terms as the term list holds them
SYSTEM = [[(700, 4), (9, ONE), (700, NEG_ONE), (700, 4), (700, 7)], [], [(12, 0)], [(5, ONE), (5, NEG_ONE), (5, 0), (6, 0)], [(1, 2), (0, 1)]]
LISTS = [[0, 1, 2, 3, 4], [1, 3], [0, 4], [1], []]


def want_items(asked):
    """ascending (position in the asked list, slot, coefficient index as an unsigned number): the specials last, a repeated term repeated"""
    return sorted((a, s, ci) for a, c in enumerate(asked) for s, ci in SYSTEM[c])


def test_shard_explain_plan_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "shard_explain_plan_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    lines = out.strip().splitlines()
    assert lines[-1] == "shard explain plan ok", out
    got = [[tuple(int(v) for v in it.split(":")) for it in ln.split()[1:]] for ln in lines if ln.startswith("items")]
    assert got == [want_items(asked) for asked in LISTS]
    assert got[0][:5] == [(0, 9, ONE), (0, 700, 4), (0, 700, 4), (0, 700, 7), (0, 700, NEG_ONE)] and got[3] == got[4] == []
    assert got[1] == [(1, 5, 0), (1, 5, NEG_ONE), (1, 5, ONE), (1, 6, 0)], "ask is the position in the asked list"
