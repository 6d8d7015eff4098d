"""The host-only pieces of lig_shard_rows_explain_attached (ligero-prover_amd/csrc/explain_plan.hpp: the layout of a rank's header block,
who holds a right-hand side, the schedule of the record all-gathers, the walk over the received records that drops the padding, the
merge into the output order with the permutation of the values, and the checks that turn a malformed block into a refusal) as a
stand-alone host program under AddressSanitizer and UBSan: no GPU, no library, nothing loaded into python.  What it checks is written
out in tests/cpp/shard_explain_attached_plan_prog.cpp; the schedules and the merged order it prints are restated here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shard_explain_attached_plan_prog.cpp")
ONE, NEG_ONE = 0xFFFFFFFF, 0xFFFFFFFE

# (the m_r of the ranks, LIG_DIAG_SLICE)
SCHEDULES = [([0, 0], 64), ([5, 0], 64), ([64, 65], 64), ([7, 200, 9], 64), ([10, 0, 33, 17], 16), ([3], 0)]
# the world of the merge cases: rank -> its (position in the asked list, global slot, coefficient index) terms
WORLD = [[(2, 90, 0), (0, 40, 2), (0, 7, ONE), (2, 3, NEG_ONE)], [(1, 55, 1), (0, 41, 0), (1, 54, 1)], [(0, 40, 2), (0, 7, 3)]]
N_ASKED = 4


def want_schedule(counts, slice_):
    M = max(counts)
    P = min(M, max(slice_, 1))
    return "schedule %s -> M %d P %d pieces %d terms %d" % (" ".join(str(c) for c in counts), M, P, -(-M // P) if M else 0, sum(counts))


def test_shard_explain_attached_plan_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "shard_explain_attached_plan_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    lines = out.strip().splitlines()
    assert lines[-1] == "shard explain attached plan ok", out
    assert [ln for ln in lines if ln.startswith("schedule")] == [want_schedule(c, s) for c, s in SCHEDULES]
    # no record all-gather when no rank holds a term; one more when the larger count passes a multiple of the slice by one
    assert want_schedule([0, 0], 64).endswith("pieces 0 terms 0") and "pieces 2" in want_schedule([64, 65], 64)
    items = [[tuple(int(v) for v in it.split(":")) for it in ln.split()[1:]] for ln in lines if ln.startswith("items")]
    want = sorted(t for rank in WORLD for t in rank)
    assert items == [want] and len(want) == 9 and want.count((0, 40, 2)) == 2, "a term two ranks hold is reported twice"
    first = [[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("first")]
    assert first == [[sum(1 for t in want if t[0] < a) for a in range(N_ASKED + 1)]] == [[0, 5, 7, 9, 9]]
