"""GPU: the three roads host rows take to the device give the same proof.  Witness rows and randomness rows of one rows job come from
host memory (lig_rows_begin / lig_rows_commit / lig_rows_prove, then lig_rows_restart + commit + prove of the same rows) with
  * the default: both through the uploader thread (arrival and consumption words in pinned host memory),
  * LIG_UPLOAD_MODE=1: witness rows by event-chained copies on the context's copy stream, randomness rows by copies on the side stream,
  * LIG_RANDS_UPLOAD_MODE=1: witness rows through the uploader thread, randomness rows by copies on the side stream.
The stream-copy roads are otherwise only reached through a retry (test_gpu_rows_api.py).  The knobs are read once per process: every
case is a child process.

The trace: l, k, n = 320, 512, 2048, 320 * 1300 + 5 linear and 330 quadratic slots = 1307 rows; stage 1 has five chunks (128, 512, 512,
59, 96), stage 2 four (192, 512, 512, 91) -- the smallest count at which the double buffer's "wait until chunk ci - 2 is consumed"
fires twice and both halves of the buffer are reused."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = textwrap.dedent('''
    import ctypes as C, json, os, sys
    import numpy as np
    sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
    import hip_lib, oracle_lib as ol
    amd = hip_lib.load()
    l, k, n = 320, 512, 2048
    job = ol.make_job(l, k, n, 192, 320 * 1300 + 5, 330, generated_at=13, threads=8)
    pr = ol.Proof()
    assert ol.lib().lo_prove(C.byref(job), C.byref(pr)) == 0
    want = bytes(pr.proof[:pr.proof_len])
    ol.lib().lo_proof_free(C.byref(pr))
    rows, _, _, _ = ol.form_rows(job)
    kinds = ol.row_kinds(job).copy()
    out = {"rows": int(len(kinds)), "proofs": [], "valid": []}
    c = amd.Context(l, k, n)
    tr, keep = c.rows_begin(kinds, rows, generated_at=13)
    for it in range(2):
        if it:
            c.rows_restart(tr, rows)
        root, seed1 = c.rows_commit(tr)
        rands, cs = ol.rand_rows(job, seed1)
        proof, info = c.rows_prove(tr, rands, cs)
        out["proofs"].append(proof == want)
        out["valid"].append([info.valid_code, info.valid_linear, info.valid_quad])
    c.trace_destroy(tr)
    out["health"] = list(c.upload_health())
    c.close()
    print(json.dumps(out))
''')


@pytest.mark.parametrize("env", [{}, {"LIG_UPLOAD_MODE": "1"}, {"LIG_RANDS_UPLOAD_MODE": "1"}], ids=["default", "upload_mode_1", "rands_upload_mode_1"])
def test_host_rows_by_every_upload_mode_equal_the_oracle(tmp_path, env):
    script = tmp_path / "upload_modes.py"
    script.write_text(CHILD)
    clean = {k: v for k, v in os.environ.items() if k not in ("LIG_UPLOAD_MODE", "LIG_RANDS_UPLOAD_MODE", "LIG_FAULT_UPLOAD")}
    p = subprocess.run([sys.executable, str(script), ROOT], env=dict(clean, **env), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert out["rows"] == 1307, out
    assert out["proofs"] == [True, True], out                  # byte for byte the oracle's envelope, first trace and restarted trace
    assert out["valid"] == [[1, 1, 1], [1, 1, 1]], out
    assert out["health"] == [0, 0], out                        # no retry, no abandoned transfer
