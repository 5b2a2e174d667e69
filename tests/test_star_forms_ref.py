"""The CPU reference of the Star family (tests/star_forms_ref.py) is held to account before it judges HIP (CPU only).

* the built form (pn + star, no auxiliary network, [256, 128, 64]) is BIT-equal to the frozen oracle/star.py;
* every form is differentiated independently by float64 autograd of a forward-only torch statement, at the bars of
  tests/test_oracle_crosscheck.py::test_star_tower_gradients_vs_float64_autograd;
* bn's forward is pn's with neutral specific tensors, and the two moving-average rules follow their closed forms;
* the idle domains' slices take the Adam step with a zero gradient.
Parity with TF 1.12 itself stays unpinned (not installable), for BatchNormalization's moving-average rule as for the rest.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import star_forms_ref as sref                       # noqa: E402
from oracle import star as ostar                    # noqa: E402
from oracle import tower as otower                  # noqa: E402
from test_oracle_crosscheck import EDGE_B, _batch, _check_grads     # noqa: E402

F32 = np.float32

# (norm, dense, auxiliary_dim, hidden): the ten combinations the GPU tests run
FORMS = [("pn", "star", 64, (256, 128, 64)), ("bn", "dense", 0, (256, 128, 64)), ("bn", "star", 64, (256, 128, 64)),
         ("pn", "dense", 64, (256, 128, 64)), ("none", "star", 0, (256, 128, 64)), ("none", "dense", 64, (256, 128, 64)),
         ("pn", "star", 64, (128, 64)), ("pn", "star", 64, (256, 128, 64, 64)), ("pn", "star", 128, (256, 128)),
         ("pn", "star", 0, (256, 128, 64))]


def perturbed(rs, n_user, n_item, n_domain, norm, dense, aux, hidden):
    """non-trivial gamma / beta / biases, Wd x 8 -- the perturbation of test_star_tower_gradients_vs_float64_autograd --
    and a non-trivial aux_b (aux_W keeps its glorot draw: no shared kernel multiplies it, x 8 would saturate the sigmoid of
    every row and leave the clip's zero gradient to check), so that the auxiliary relu is active on a real share of its units."""
    p = sref.init_params(rs, n_user, n_item, n_domain, hidden, norm, dense, aux)
    for n in ("pn_gamma_shared", "pn_gamma_spec", "bn_gamma"):
        if n in p:
            p[n] = (p[n] + rs.standard_normal(p[n].shape) * 0.2).astype(F32)
    for n in list(p):
        if n in ("pn_beta_shared", "pn_beta_spec", "bn_beta", "gb", "aux_b") or n[:2] in ("bs", "bd") or \
                (n[0] == "b" and n[1:].isdigit()):
            p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
    for n in list(p):
        if n[:2] == "Wd":
            p[n] = (p[n] * 8).astype(F32)
    return p


@pytest.mark.parametrize("emb_trainable", [False, True])
def test_built_form_is_bit_equal_to_the_frozen_oracle(emb_trainable):
    rs = np.random.RandomState(12)
    n_user, n_item, n_domain, B = 300, 200, 4, 192
    p = ostar.init_params(rs, n_user, n_item, n_domain)
    for n in ("pn_gamma_shared", "pn_gamma_spec"):
        p[n] = (p[n] + rs.standard_normal(p[n].shape) * 0.2).astype(F32)
    for n in ("pn_beta_shared", "pn_beta_spec", "bs0", "bs1", "bs2", "bd0", "bd1", "bd2", "gb"):
        p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
    for l in range(3):
        p["Wd%d" % l] = (p["Wd%d" % l] * 8).astype(F32)
    uid, pid, dom, label = _batch(rs, n_user, n_item, n_domain, B, single_domain=1)
    assert sref.param_names(emb_trainable) == ostar.param_names(emb_trainable)
    a = ostar.OracleStar({k: v.copy() for k, v in p.items()}, emb_trainable=emb_trainable)
    b = sref.StarForms({k: v.copy() for k, v in p.items()}, emb_trainable=emb_trainable)
    la, ga, pa, _ = ostar.loss_and_grads(a.params, a.state, uid, pid, dom, label, emb_trainable)
    lb, gb, pb, _ = b.loss_and_grads(uid, pid, dom, label)
    assert la.tobytes() == lb.tobytes() and pa.tobytes() == pb.tobytes()
    for n in a.names:
        assert np.asarray(ga[n]).tobytes() == np.asarray(gb[n]).tobytes(), n
    for _ in range(3):
        assert a.train_on_batch(uid, pid, dom, label).tobytes() == b.train_on_batch(uid, pid, dom, label).tobytes()
    assert a.get_flat().tobytes() == b.get_flat().tobytes()
    for k in a.state:
        assert a.state[k].tobytes() == b.state[k].tobytes(), k


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("norm,dense,aux,hidden", FORMS)
def test_forms_gradients_vs_float64_autograd(norm, dense, aux, hidden, mixed):
    _forms_case(norm, dense, aux, hidden, mixed, 192)


# gb is the sum of (p - y) / B over 2 or 3 rows of both labels, which cancels to 1e-3 of its terms on these draws (see
# test_oracle_crosscheck.EDGE_SEEDS): another seed, the same bars
FORMS_EDGE_SEEDS = {("pn", "dense", 64, (256, 128, 64), False, 2): 13, ("pn", "star", 128, (256, 128), False, 3): 13}


@pytest.mark.parametrize("B", EDGE_B)
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("norm,dense,aux,hidden", FORMS)
def test_forms_gradients_vs_float64_autograd_at_edge_batches(norm, dense, aux, hidden, mixed, B):
    _forms_case(norm, dense, aux, hidden, mixed, B, FORMS_EDGE_SEEDS.get((norm, dense, aux, hidden, mixed, B), 12))


@pytest.mark.parametrize("mixed", [False, True], ids=["one-domain", "mixed"])
@pytest.mark.parametrize("n_domain", [1, 33, 65])
@pytest.mark.parametrize("norm,dense,aux,hidden", [FORMS[0], FORMS[9]])
def test_forms_gradients_vs_float64_autograd_at_edge_domain_counts(norm, dense, aux, hidden, n_domain, mixed):
    """pn + star with and without the auxiliary network at 1, 33 and 65 domains (tests/test_gpu_domain_counts.py runs the
    step kernels' Star and the generic-layer engine there): 256 rows of the highest domain id, and 256 rows in which every
    id occurs, led by the highest (the first row's domain serves the batch).  One input was moved: pn/star/64 at 33 domains,
    one-domain, seed 12 puts a hidden unit within fp32 rounding of the relu kink (user_emb off by 7.6e-5 of 0.073 on 0.6 % of
    its elements, the signature of one flipped unit); seed 13, the same bars."""
    seed = {("pn", "star", 64, 33, False): 13}.get((norm, dense, aux, n_domain, mixed), 12)
    _forms_case(norm, dense, aux, hidden, mixed, 256, seed, n_domain=n_domain, domain=n_domain - 1)


@pytest.mark.parametrize("n_domain", [1, 33])
def test_domain_count_star_form_inputs(n_domain):
    """the batches tests/test_gpu_domain_counts.py probes with pn/star/64 on the generic-layer engine, through the reference
    alone.  That file applies tests/test_gpu_star_forms.py::fit_reference per batch, so a batch at the kink is judged by
    float64 there; here the distance is measured and every tensor off the kink's signature is held to `_check_grads`."""
    import domain_counts as dc
    g = dc.star_form_problem(n_domain)
    rs = np.random.RandomState(11)
    p = perturbed(rs, g["n_user"], g["n_item"], n_domain, "pn", "star", 64, (256, 128, 64))
    p["user_emb"], p["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    meta, rest = sref.param_names(False, "pn", "star", 64, 3)
    names = meta + rest
    for d, args in dc.probe_batches(g):
        state = sref.init_state("pn", n_domain)
        loss32, g32, p32, _ = sref.loss_and_grads(p, state, *args, False, "pn", "star", 64)
        loss64, g64, p64, _ = sref.loss_and_grads64(p, names, *args, "pn", "star", 64)
        assert abs(float(loss32) - loss64) < 2e-6 * max(1.0, abs(loss64))
        np.testing.assert_allclose(p32, p64, rtol=5e-5, atol=5e-7)
        assert np.all(args[2] == d)
        _check_grads(g32, g64, [n for n in names if n != "domain_emb"], rtol=1e-3)


def _forms_case(norm, dense, aux, hidden, mixed, B, seed=12, n_domain=4, domain=1):
    rs = np.random.RandomState(seed)
    n_user, n_item = 300, 200
    p = perturbed(rs, n_user, n_item, n_domain, norm, dense, aux, hidden)
    uid, pid, dom, label = _batch(rs, n_user, n_item, n_domain, B, single_domain=None if mixed else domain)
    if mixed and n_domain != 4:             # every id occurs, the highest first
        dom = np.concatenate([[n_domain - 1], rs.permutation(np.arange(1, B) % n_domain)]).astype(np.int32)
    d = int(dom[0])
    meta, rest = sref.param_names(True, norm, dense, aux, len(hidden))
    names = meta + rest
    state = sref.init_state(norm, n_domain)
    loss32, g32, p32, c = sref.loss_and_grads(p, state, uid, pid, dom, label, True, norm, dense, aux)
    loss64, g64, p64, extra = sref.loss_and_grads64(p, names, uid, pid, dom, label, norm, dense, aux)
    print("%s/%s/aux %d/%r mixed=%s: loss %.3e" % (norm, dense, aux, hidden, mixed, abs(float(loss32) - loss64)))
    assert abs(float(loss32) - loss64) < 2e-6 * max(1.0, abs(loss64))
    np.testing.assert_allclose(p32, p64, rtol=5e-5, atol=5e-7)
    if norm != "none":
        np.testing.assert_allclose(c["mean"], extra["mean"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(c["var"], extra["var"], rtol=1e-5, atol=1e-9)
    if aux:         # a condition on the inputs, not a tolerance: the auxiliary relu is neither dead nor the identity
        active = float(np.mean(c["a"] > 0))
        print("auxiliary relu active on %.1f %% of units" % (100 * active))
        assert 0.10 < active < 0.90
    check = list(names)
    if norm != "none" and len(np.unique(dom)) == 1:        # (not mixed, or 2 - 3 mixed rows that drew one domain)
        # the domain row is constant over a single-domain batch: the norm maps it to beta, its gradient is rounding
        # residue in fp32 and ~0 in float64 (under `none` it is a real gradient and checked like any tensor)
        assert np.abs(g32["domain_emb"]).max() < 1e-5 and np.abs(g64["domain_emb"]).max() < 1e-5
        check.remove("domain_emb")
    _check_grads(g32, g64, check, rtol=1e-3)
    for n in ("Wd0", "bd1", "pn_gamma_spec", "aux_W", "aux_b"):      # the other domains' slices: exactly zero on both sides
        if n in names:
            for j in range(n_domain):
                if j != d:
                    assert not np.any(g32[n][j]) and not np.any(g64[n][j]), (n, j)


def test_bn_forward_is_pn_forward_with_neutral_specific_tensors():
    rs = np.random.RandomState(5)
    n_user, n_item, n_domain, B = 120, 90, 3, 64
    pp = perturbed(rs, n_user, n_item, n_domain, "pn", "star", 64, (256, 128, 64))
    pp["pn_gamma_spec"][...] = 1
    pp["pn_beta_spec"][...] = 0
    pb = {k: v for k, v in pp.items() if not k.startswith("pn_")}
    pb["bn_gamma"], pb["bn_beta"] = pp["pn_gamma_shared"], pp["pn_beta_shared"]
    uid, pid, dom, label = _batch(rs, n_user, n_item, n_domain, B, single_domain=2)
    a, _ = sref.forward(pp, sref.init_state("pn", n_domain), uid, pid, dom, True, "pn", "star", 64)
    b, _ = sref.forward(pb, sref.init_state("bn", n_domain), uid, pid, dom, True, "bn", "star", 64)
    assert a.tobytes() == b.tobytes()


def test_moving_average_rules_follow_their_closed_forms():
    """a constant input: pn (zero-debiased) shows the value itself from step 1 on, bn (plain) value (1 - 0.99^k)."""
    mean, var = np.full(384, 0.37, F32), np.full(384, 2.5, F32)
    pn, bn = sref.init_state("pn", 3), sref.init_state("bn", 3)
    for k in range(1, 8):
        sref.update_moving(pn, "pn", 1, mean, var)
        sref.update_moving(bn, "bn", 1, mean, var)
        np.testing.assert_allclose(pn["mov_mean"][1], mean, rtol=3e-6)
        np.testing.assert_allclose(pn["mov_var"][1], var, rtol=3e-6)
        np.testing.assert_allclose(bn["mov_mean"], 0.37 * (1 - 0.99 ** k), rtol=3e-6)
        np.testing.assert_allclose(bn["mov_var"], 0.99 ** k + 2.5 * (1 - 0.99 ** k), rtol=3e-6)      # (starts at one)
        assert pn["steps"][1] == k and not np.any(pn["mov_mean"][0]) and np.all(pn["mov_var"][2] == 1)


def test_idle_slices_take_the_adam_step_with_a_zero_gradient():
    rs = np.random.RandomState(7)
    n_user, n_item, n_domain, B = 120, 90, 3, 64
    p = perturbed(rs, n_user, n_item, n_domain, "pn", "star", 64, (256, 128, 64))
    m = sref.StarForms(p, "pn", "star", 64, emb_trainable=False)
    for n in ("aux_W", "Wd0"):
        m.opt.m[n][...] = (rs.standard_normal(p[n].shape) * 1e-2).astype(F32)
        m.opt.v[n][...] = (rs.uniform(1e-6, 1e-4, p[n].shape)).astype(F32)
    twin = {n: {"p": p[n].copy(), "m": m.opt.m[n].copy(), "v": m.opt.v[n].copy()} for n in ("aux_W", "Wd0")}
    ref = otower.Optimizer({n: twin[n]["p"] for n in twin}, tuple(twin))
    for n in twin:
        ref.m[n][...], ref.v[n][...] = twin[n]["m"], twin[n]["v"]
    uid, pid, dom, label = _batch(rs, n_user, n_item, n_domain, B, single_domain=1)
    before = {n: p[n].copy() for n in twin}
    for _ in range(3):
        m.train_on_batch(uid, pid, dom, label)
        ref.adam({n: twin[n]["p"] for n in twin}, {n: np.zeros_like(twin[n]["p"]) for n in twin}, 1e-3)
    for n in twin:
        for j in (0, 2):
            assert np.any(p[n][j] != before[n][j]), n                      # decayed momentum moves them: not frozen
            assert p[n][j].tobytes() == twin[n]["p"][j].tobytes(), n       # ... exactly as a zero gradient does
        assert np.any(p[n][1] != twin[n]["p"][1])
