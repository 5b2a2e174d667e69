"""The config scalars `dropout`, `l2_emb`, `l2_linear` off their coinciding defaults, on the CPU: the TEETH of
tests/test_gpu_config_scalars.py's comparison (mutated oracles against the true one, with that file's helper, values and
shapes), the pinned dropout scalars of oracle/rng.py, and the config -> engine-constructor plumbing of the rate.

Plumbing not repeated here: a Star config with `"dropout": 0.5` reaching the engine with 0.0 is asserted by
tests/test_host_logic.py::test_star_plain_dnn_form (the stand-in's oracle) and by every Star row of
tests/test_embdim_host.py::test_routing_table (the constructor's keyword).
"""
import numpy as np
import pytest

import config_scalars as cs
from oracle import rng as orng

F32 = np.float32
# one check per oracle family member; trainable tables where the GPU file has a trainable case of the kind
CASES = [("mlp", True), ("deepfm", True), ("wdl", False), ("nfm", True), ("pnn", False), ("ccpm", False), ("autoint", False),
         ("shared_bottom", True), ("mmoe", False), ("ple", False)]
TABLE = []          # (kind, mutant, rate, {tensor: fraction beyond the bar}, loss / bar): printed once, profiles/config_scalars.txt


@pytest.fixture(scope="module", autouse=True)
def _print_table():
    yield
    for kind, mutant, rate, frac, loss in TABLE:
        print("MUTANT %-13s %-18s rate %.2f loss %9.1f x bar | %s" % (kind, mutant, rate, loss,
                                                                    " ".join("%s %.2f" % kv for kv in sorted(frac.items()))))


@pytest.mark.parametrize("kind,emb_trainable", CASES)
def test_mutated_oracles_are_rejected_and_the_defaults_are_blind(kind, emb_trainable):
    """every mutant against the true oracle through the GPU file's helper: l2 swapped, either weight dropped (at the pair
    L2), keep scale from 1 / rate, mask from u >= (1 - rate) 2^32 (at both rates) -- each on every tensor that carries the
    term, on the pass's full first batch and its partial last one.  Floors: the read-back ulp of each tensor, as on the
    GPU.  Then the blind spot, written down: at the defaults (1e-5, 1e-5) the swap mutant PASSES the same helper, and at
    rate 1/2 the keep-scale mutant's numbers are the true oracle's, bit for bit."""
    for rate in cs.RATES:
        P = cs.Problem(kind, emb_trainable, rate=rate)
        floors = {n: cs.ulp_floor(P.params[n]) for n in P.names}
        for step in (0, P.n_step - 1):
            loss, want = P.grads(step, step)
            touched = P.touched(step)
            assert cs.Report(want, want, loss, loss, floors).ok()
            mutants = {}
            if rate == cs.RATES[0]:                 # (the regularisers do not depend on the rate)
                for name, pair in cs.l2_mutants(cs.L2).items():
                    mutants[name] = P.grads(step, step, l2=tuple(F32(x) for x in pair))
            for which in ("keep_scale", "mask"):
                with cs.mutated(which):
                    mutants["%s mutant" % which] = P.grads(step, step)
            for name, (mloss, got) in mutants.items():
                dropout = name.endswith("mutant")
                rep = cs.Report(got, want, mloss, loss, floors, select=touched if dropout else None)
                names = cs.carriers(P, name, want)
                if step == 0:
                    TABLE.append((kind, name, rate, {n: rep.frac[n] for n in names}, rep.loss))
                assert rep.ok() == (not names), (kind, name, rate, step)       # (no linear table: l2_linear is no term of this tower)
                for n in names:
                    assert rep.rejected(n), (kind, name, rate, step, n, rep)
                if not dropout:                     # ... and nothing else moved: the mutant is the term, not a side effect
                    assert not any(v for n, v in rep.frac.items() if n not in names), (kind, name, rep)
    # the blind spot at the defaults
    P = cs.Problem(kind, emb_trainable, rate=0.5, l2=cs.DEFAULT_L2)
    loss, want = P.grads(0, 0)
    floors = {n: cs.ulp_floor(P.params[n]) for n in P.names}
    mloss, got = P.grads(0, 0, l2=(F32(cs.DEFAULT_L2[1]), F32(cs.DEFAULT_L2[0])))
    rep = cs.Report(got, want, mloss, loss, floors)
    assert rep.ok() and rep.loss == 0.0
    with cs.mutated("keep_scale"):
        mloss, got = P.grads(0, 0)
    assert mloss == loss and all(np.array_equal(got[n].view(np.uint32), want[n].view(np.uint32)) for n in want)
    with cs.mutated("mask"):
        mloss, got = P.grads(0, 0)
    assert mloss == loss and all(np.array_equal(got[n].view(np.uint32), want[n].view(np.uint32)) for n in want)
    # l2 None keeps the oracle's constants, bit for bit
    mloss, got = P.grads(0, 0, model=P.make_model(None))
    assert mloss == loss and all(np.array_equal(got[n].view(np.uint32), want[n].view(np.uint32)) for n in want)


def test_reported_and_evaluation_losses_carry_the_pair():
    """the l2 argument reaches the reported loss and the evaluation loss of every oracle class, not the gradients alone."""
    for kind in ("deepfm", "nfm", "autoint", "mmoe"):
        P = cs.Problem(kind, False, rate=0.25)
        val = P.g["data"]["val"][P.d]
        ev = lambda m: float(m.evaluate(P.d, val, 256)[0] if P.family == "mtl" else m.evaluate(val, 256)[0])     # noqa: E731
        base, swapped, none = ev(P.model), ev(P.make_model((cs.L2[1], cs.L2[0]))), ev(P.make_model(None))
        assert cs.loss_excess(swapped, base) > 10, (kind, base, swapped)
        assert none == ev(P.make_model(cs.DEFAULT_L2)), kind
        b = P.batch(0)
        args = (P.d,) if P.family == "mtl" else ()
        losses = [float(m.train_on_batch(*args, b["uid"], b["pid"], b["domain"], b["label"]))
                  for m in (P.make_model(cs.L2), P.make_model((cs.L2[1], cs.L2[0])))]
        assert cs.loss_excess(losses[1], losses[0]) > 10, (kind, losses)


def test_dropout_scalars_are_the_librarys():
    """threshold and keep scale from np.float32(rate), the value that crosses the ABI (mamdr_train_steps_n,
    mamdr_graph_train_steps_n: `(double)rate * 2^32` truncated, `(float)(1 / (1 - (double)rate))`)."""
    assert int(orng.dropout_threshold(0.25)) == 2 ** 30
    assert int(orng.dropout_threshold(0.75)) == 3 * 2 ** 30
    assert int(orng.dropout_threshold(0.5)) == 2 ** 31
    assert int(orng.dropout_threshold(0.1)) == 429496736            # (the Python double's 0.1 gives 429496729)
    assert int(float(0.1) * 4294967296.0) == 429496729
    assert int(orng.dropout_threshold(0.0)) == 0
    assert orng.dropout_mask(3, 5, 1, 37, 19, 0.0).all()
    assert (orng.dropout_u32(3, 5, 1, 37, 19) >= orng.dropout_threshold(0.0)).all()
    ks = orng.keep_scale(0.25)
    assert ks.dtype == np.float32 and ks == F32(1.0 / 0.75) and orng.keep_scale(0.75) == F32(4) and orng.keep_scale(0.5) == F32(2)
    assert orng.keep_scale(0.1) == F32(1.0 / (1.0 - float(F32(0.1)))) and orng.keep_scale(0.0) == F32(1)
    # the mask keeps 1 - rate of the stream
    for rate in cs.RATES:
        kept = orng.dropout_mask(1024, 0, 0, 256, 256, rate).mean()
        assert abs(kept - (1.0 - rate)) < 0.01, (rate, kept)


@pytest.mark.parametrize("name,extra,factory", [
    ("mlp_meta_mamdr_finetune", {}, "tower"),
    ("nfm", {}, "tower"),
    ("mmoe", {"hidden_dim": [16, 8], "tower_hidden_dim": [4], "num_experts": 2, "gate_dnn_hidden_units": [4]}, "graph")])
def test_config_dropout_reaches_the_engine_constructor(tmp_path, monkeypatch, name, extra, factory):
    """a DeepCTR config (step-engine route and generic-layer route) and a DeepMTLCTR config with `"dropout": 0.25`: the
    stand-in engine is constructed with 0.25."""
    from fake_engine import FakeEngine, FakeGraphEngine
    from mamdr_amd import cli
    from mamdr_amd.utils import dataset as mds
    from test_host_logic import patch_emb_dim, tiny_config
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, name, epochs=1)
    cfg["model"].update(dropout=0.25, **extra)
    model = cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), FakeEngine if factory == "tower" else FakeGraphEngine)
    assert model.model.oracle.rate == 0.25
