"""CPU: the exact integer model of the 29-bit-limb field core (tools/check_fr29.py) holds at the corners of the operand ranges
csrc/fr29.hpp states, with the constants of the committed csrc/fr29_consts.hpp and the column tables of tools/gen_fr29_montmul.py;
and the model itself notices the mistakes it is there for."""
import importlib.util
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("check_fr29", os.path.join(ROOT, "tools", "check_fr29.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_core_model_holds_at_the_stated_bounds():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_fr29.py")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) > 1 and all(ln.startswith("ok: ") for ln in lines) and lines[-1] == "ok: all checks passed"
    for name in ("f29_montmul", "f29_qnorm", "f29_reduce_2p", "f29_canon", "K2P/K4P/K8P/K16P", "unpack29 / pack29"):
        assert any(name in ln for ln in lines), name


def test_model_reads_the_committed_constants(model):
    with open(os.path.join(ROOT, "ligero-prover_amd", "csrc", "fr29_consts.hpp")) as f:
        text = f.read()
    for name in ("F29_P", "F29_PBAR", "F29_K2P_C1", "F29_K4P_C2", "F29_K8P_C4", "F29_K16P_C2", "F29_R2", "F29_ONE_M"):
        assert len(model.K[name]) == 9 and all("0x%08Xu" % v in text for v in model.K[name]), name
    for name in ("F29_N0", "F29_RECIP229", "F29_MASK"):
        assert "#define %s 0x%08Xu" % (name, model.K[name]) in text
    assert model.value(model.K["F29_P"]) == model.P


def test_model_notices_a_longer_renormalisation_interval_and_a_short_quotient(model, monkeypatch):
    """the model is not vacuous: 8 all-ones terms between two carry passes overflow a 32-bit limb in the second interval, and
    with a reciprocal that is 2^25 (1.5 %) too small the quotient estimate is more than one short somewhere in the sweep"""
    m = model
    term = m.norm((((m.P >> 232) - 1) << 232) | ((1 << 232) - 1))
    a = [0] * 9
    with pytest.raises(AssertionError, match="32 bits"):
        for i in range(16):
            a = [m.u32(x + y) for x, y in zip(a, term)]
            if i % 8 == 7:
                a = m.qnorm(a)
    m.reduce_2p(m.norm((1 << 261) - 1))
    monkeypatch.setattr(m, "RECIP229", m.RECIP229 - (1 << 25))
    with pytest.raises(AssertionError):
        m.check_reduce(random.Random(1))


def test_montmul_model_is_the_all_ones_product(model):
    """the (u, r) pairs of tests/extremal.py: the device product is exactly the all-ones value"""
    import numpy as np
    import extremal as ex
    import oracle_lib as ol
    u, r = ex.allones_products(50, np.random.default_rng(3))
    for a, b in zip(ol.from_limbs(u), ol.from_limbs(r)):
        t = model.montmul(model.unpack29(model.words(a)), model.unpack29(model.words(b)))
        assert t == [model.MASK] * 8 + [(model.P >> 232) - 1]
