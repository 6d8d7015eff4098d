"""The host-only pieces of lig_shard_rows_explain_slots* / lig_shard_rows_untouched_slots* (ligero-prover_amd/csrc/explain_plan.hpp: which
asked slots a rank holds, the layout of a rank's header block, the one holder of a slot, the piece schedule of the item all-gathers, the
walk over the received items with its refusals, and the W-way merge of the untouched lists with the cut at cap) as a stand-alone host
program under AddressSanitizer and UBSan: no GPU, no library, nothing loaded into python.  What it checks is written out in
tests/cpp/shard_slots_plan_prog.cpp; the schedules, the ordered items and the merged lists it prints are restated here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shard_slots_plan_prog.cpp")
ONE, NEG_ONE = 0xFFFFFFFF, 0xFFFFFFFE

# the statement of the program's world but for the 70 terms of slot 14: (slot, constraint, coefficient index)
STATEMENT = [(3, 9, 2), (3, 4, ONE), (3, 4, 1), (3, 4, 1), (12, 9, 0), (35, 1, NEG_ONE), (35, 0, 5), (41, 9, 2), (59, 7, 3), (59, 2, 3), (21, 4, 0)]
ASKED = [3, 12, 14, 21, 30, 35, 41, 59]
COUNTS = [6, 74, 1]                                    # the m_r of the three ranks
# the untouched lists of four ranks, one of them empty
LISTS = [[5, 6, 7, 30, 31, 90], [], [1, 2, 8, 9, 40, 41, 42, 43, 44], [3, 100]]


def want_schedule(slice_, counts):
    M = max(counts)
    P = min(M, max(slice_, 1))
    return "schedule slice %d -> M %d P %d pieces %d terms %d" % (slice_, M, P, -(-M // P) if M else 0, sum(counts))


def test_shard_slots_plan_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "shard_slots_plan_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    lines = out.strip().splitlines()
    assert lines[-1] == "shard slots plan ok", out
    # one piece; m_r exactly P; two pieces of 37; three pieces with a ragged last one (74 = 2 * 32 + 10); one item per piece; slice 0 reads as 1;
    # then m_r = {6, 2, 0}: the largest rank fills the one piece exactly; and no term at all: no piece
    want = [want_schedule(s, COUNTS) for s in (1 << 20, 74, 37, 32, 1, 0)] + [want_schedule(6, [6, 2, 0]), want_schedule(64, [0, 0, 0])]
    assert [ln for ln in lines if ln.startswith("schedule")] == want
    assert want[1].endswith("P 74 pieces 1 terms 81") and want[3].endswith("P 32 pieces 3 terms 81") and want[7].endswith("P 0 pieces 0 terms 0")
    # the output order: asked slot, constraint, coefficient index as an unsigned number; a repeated term twice (slot 14's 70 terms left out)
    items = [[tuple(int(v) for v in it.split(":")) for it in ln.split()[1:]] for ln in lines if ln.startswith("items")]
    order = sorted((ASKED.index(s), c, ci) for s, c, ci in STATEMENT)
    assert items == [order] and order[:4] == [(0, 4, 1), (0, 4, 1), (0, 4, ONE), (0, 9, 2)]
    first = [[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("first")]
    n_terms = [sum(1 for s, _, _ in STATEMENT if s == a) + (70 if a == 14 else 0) for a in ASKED]
    assert first == [[sum(n_terms[:a]) for a in range(len(ASKED) + 1)]] and first[0][-1] == sum(COUNTS)
    # the merge: the first cap of all the lists, ascending, whatever the pieces were
    every = sorted(s for li in LISTS for s in li)
    merged = {int(ln.split()[2]): [int(v) for v in ln.split()[5:]] for ln in lines if ln.startswith("merge cap")}
    assert merged == {cap: every[:cap] for cap in (0, 1, 4, 9, 16, 17, 22)} and len(every) == 17
