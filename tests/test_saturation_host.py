"""tests/saturation.py on the CPU: the row selection holds its conditions on every oracle the GPU tests of
tests/test_gpu_saturation.py use, the clipped rows' loss is the four constants, and the oracle's clip gate (`inside`) agrees
with float64 autograd of oracle/torch_ref.py's clamped BCE on a mixed batch -- the reference is validated in this regime
here, without a GPU.

The problems restate the `make_problem` recipes of the GPU test modules (they build an engine, which needs a device): same
synthetic data, same seeds, same perturbations of the initial values.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import saturation as sat                            # noqa: E402
from oracle import tower as otower                  # noqa: E402

F32 = np.float32
H3 = (256, 128, 64)
# (route, dropout rates): every engine kind of tests/test_gpu_saturation.py's coverage table
ROUTES = [("mlp", (0.5, 0.0)), ("deepfm", (0.5, 0.0)), ("pnn", (0.5, 0.0)), ("nfm", (0.5, 0.0)), ("mlp-trainable", (0.5,)),
          ("deepfm-trainable", (0.5,)), ("mlp-uncertainty", (0.5,)), ("star", (0.0,)), ("graph-mlp", (0.5,)),
          ("autoint", (0.5,)), ("mmoe", (0.5,)), ("starform", (0.0,))]


def largest(g):
    return max(range(g["n_domain"]), key=lambda k: g["data"]["train"][k]["uid"].shape[0])


def host_problem(route, dropout):
    """the oracle side of the GPU tests' problems -> saturation.Problem over the largest domain's train split."""
    from mamdr_amd import synthetic
    kind, _, opt = route.partition("-")
    trainable, uncertainty = opt == "trainable", opt == "uncertainty"
    if route == "mmoe":                                 # tests/test_gpu_mtl.py:make_problem
        from oracle import mtl as omtl
        g = synthetic.generate(dict(synthetic.SHAPES["taobao10"], n_domain=4), batch_size=24, seed=7, scale=0.05)
        spec = omtl.Spec("mmoe", 4, (128, 64), (64,), (64,), num_experts=3)
        rs = np.random.RandomState(7)
        p = omtl.init_params(rs, spec, g["n_user"], g["n_item"])
        p["user_emb"], p["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
        for n in p:
            if "/b" in n or n.endswith("/gb") or n == "domain_emb":
                p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
        d = largest(g)
        return sat.Problem("mtl", omtl.OracleMTL(p, spec, dropout=dropout, lr=1e-3), g["data"]["train"][d], d, spec)
    if route in ("star", "starform"):
        g = synthetic.generate("taobao10", batch_size=24, seed=11, scale=0.05)
        rs = np.random.RandomState(11)
        d = largest(g)
        if route == "star":                             # tests/test_gpu_parity.py:make_star_problem
            from oracle import star as ostar
            p = ostar.init_params(rs, g["n_user"], g["n_item"], g["n_domain"])
            p["user_emb"], p["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
            for n in ("pn_gamma_shared", "pn_gamma_spec"):
                p[n] = (p[n] + rs.standard_normal(p[n].shape) * 0.2).astype(F32)
            for n in ("pn_beta_shared", "pn_beta_spec", "bs0", "bs1", "bs2", "bd0", "bd1", "bd2", "gb"):
                p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
            for l in range(3):
                p["Wd%d" % l] = (p["Wd%d" % l] * 8).astype(F32)
            return sat.Problem("star", ostar.OracleStar(p, emb_trainable=False, lr=1e-3), g["data"]["train"][d], d)
        import star_forms_ref as sref                   # tests/test_gpu_star_forms.py:build
        from test_star_forms_ref import perturbed
        p = perturbed(rs, g["n_user"], g["n_item"], g["n_domain"], "pn", "star", 64, H3)
        p["user_emb"], p["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
        return sat.Problem("starform", sref.StarForms(p, "pn", "star", 64, emb_trainable=False), g["data"]["train"][d], d)
    g = synthetic.generate("taobao10", batch_size=24, seed=7, scale=0.05)
    rs = np.random.RandomState(7)
    d = largest(g)
    if kind in ("pnn", "nfm", "autoint"):               # tests/test_gpu_fmnets.py:make_problem
        from oracle import fmnets as ofm
        if kind == "autoint":
            p = ofm.init_params_conv(rs, kind, g["n_user"], g["n_item"], g["n_domain"], hidden=H3)
            for l in range(3):
                p["att%d_w" % l] = (p["att%d_w" % l] * 4).astype(F32)
        else:
            p = ofm.init_params(rs, kind, g["n_user"], g["n_item"], g["n_domain"], hidden=H3)
        p["user_emb"], p["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
        p["domain_emb"] = (rs.standard_normal(p["domain_emb"].shape) * 0.05).astype(F32)
        for n in ("b0", "b1", "b2", "lin_domain", "lin_user", "lin_item"):
            p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
        p["gb"] = np.array([0.1], F32)
        p["lin_user"][...] = 0
        p["lin_item"][...] = 0
        return sat.Problem("fm", ofm.OracleNet(p, kind, dropout=dropout, lr=1e-3, hidden=H3), g["data"]["train"][d], d)
    if kind == "graph":                                 # tests/test_gpu_hidden.py:make_problem, hidden [128, 64]
        hidden = (128, 64)
        p = otower.init_params(rs, g["n_user"], g["n_item"], g["n_domain"], hidden=hidden)
        p["user_emb"], p["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
        p["domain_emb"] = (rs.standard_normal(p["domain_emb"].shape) * 0.05).astype(F32)
        for n in ["b0", "b1", "lin_domain", "lin_user", "lin_item"]:
            p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
        p["gb"] = np.array([0.1], F32)
        model = otower.OracleModel(p, dropout=dropout, lr=1e-3, hidden=hidden, tower="mlp")
        return sat.Problem("tower", model, g["data"]["train"][d], d)
    # tests/test_gpu_parity.py:make_problem
    p = otower.init_params(rs, g["n_user"], g["n_item"], g["n_domain"])
    p["user_emb"], p["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    p["domain_emb"] = (rs.standard_normal(p["domain_emb"].shape) * 0.05).astype(F32)
    for l in range(3):
        p["b%d" % l] = (rs.standard_normal(p["b%d" % l].shape) * 0.05).astype(F32)
    if kind == "deepfm":
        p["lin_domain"] = (rs.standard_normal(g["n_domain"]) * 0.05).astype(F32)
        if trainable:
            p["lin_user"] = (rs.standard_normal(g["n_user"]) * 0.05).astype(F32)
            p["lin_item"] = (rs.standard_normal(g["n_item"]) * 0.05).astype(F32)
    if uncertainty:
        p["log_var"] = (1.0 + rs.uniform(-0.3, 0.3, g["n_domain"])).astype(F32)
    model = otower.OracleModel(p, emb_trainable=trainable, dropout=dropout, lr=1e-3, tower=kind, uncertainty=uncertainty)
    return sat.Problem("tower", model, g["data"]["train"][d], d)


@pytest.mark.parametrize("route,dropout", [(r, rate) for r, rates in ROUTES for rate in rates])
def test_selection_holds_its_conditions(route, dropout):
    """the mixed batch of 24 rows (8 normal, 16 saturated or extreme, every clipped class with both labels, nothing in
    6 < |z| < 20), the all-saturated batches of 5 rows and of 1 row, and a 24-row evaluation split, on every oracle: `pick`
    asserts the conditions itself; here they are asserted again on logits recomputed from scratch."""
    prob = host_problem(route, dropout)
    z_all, guess = sat.saturate(prob)
    assert z_all.min() < -100 and z_all.max() > 100
    labels = prob.cols["label"]
    taken, step = [], 0
    for layout in (sat.MIXED, sat.ALL_SATURATED_5, sat.ALL_SATURATED_1):
        step, idx, z = sat.pick(prob, layout, step, guess=guess, exclude=taken)
        taken += list(idx)
        z2 = prob.loss_and_grads(idx, step)[2]
        step += 1
        assert np.array_equal(z, z2) and len(set(idx.tolist())) == len(layout)
        a = np.abs(z2.astype(np.float64))
        assert not np.any((a > 6) & (a < 20)) and np.all(a <= 1000)
        y = labels[idx]
        if layout is sat.MIXED:
            assert int((a <= 6).sum()) == 8
            for lo, hi in ((20, 80), (100, 1000)):
                for sign in (1, -1):
                    rows = (sign * z2 >= lo) & (sign * z2 <= hi)
                    assert set(y[rows].astype(int).tolist()) == {0, 1}, (lo, sign)
        else:
            assert np.all(a >= 20)
            wrong = ((z2 > 0) & (y == 0)) | ((z2 < 0) & (y == 1))
            assert wrong[0] and wrong[-1]
    # the evaluation split: the same classes under the INFERENCE logits (no dropout, a norm layer's moving statistics)
    prob = host_problem(route, dropout)
    sat.saturate(prob, inference=True)
    idx, z = sat.pick_eval(prob, prob.cols, sat.MIXED)
    a = np.abs(z.astype(np.float64))
    assert int((a <= 6).sum()) == 8 and not np.any((a > 6) & (a < 20))


def test_clipped_rows_have_the_four_constant_losses():
    """fp32 facts the GPU tests rest on: hi = 1 - 2^-23, the oracle's sigmoid is inside the clip for -16.118 <= z <= 16.63
    and jumps from 1 - 2^-23 straight to 1.0, and a clipped row's loss is one of four constants."""
    hi = F32(1) - otower.EPS_CLIP
    assert hi == F32(1 - 2.0 ** -23) and otower.EPS_CLIP == F32(1e-7)
    z = np.array([-1000, -100, -80, -20, 20, 80, 100, 1000], F32)
    p = otower.sigmoid(z)
    assert np.all(p[4:] == 1.0) and np.all(p[:4] < 1e-7) and p[0] == 0.0
    l0, l1 = otower.bce_per_row(p, np.zeros(8, F32)), otower.bce_per_row(p, np.ones(8, F32))
    np.testing.assert_allclose(l0[4:], sat.LOSS_HIGH_Y0, rtol=1e-5)
    np.testing.assert_allclose(l1[4:], sat.LOSS_HIGH_Y1, rtol=5e-3)
    np.testing.assert_allclose(l1[:4], sat.LOSS_LOW_Y1, rtol=1e-5)
    np.testing.assert_allclose(l0[:4], sat.LOSS_LOW_Y0, rtol=5e-3)
    assert len(set(l0[4:].tolist())) == len(set(l1[:4].tolist())) == 1       # constants: the same bits at every such logit
    inside = (otower.sigmoid(np.array([-16.118, 16.63], F32)) >= otower.EPS_CLIP) & \
        (otower.sigmoid(np.array([-16.118, 16.63], F32)) <= hi)
    assert inside.all()
    grid = otower.sigmoid(np.arange(15.0, 17.5, 0.001).astype(F32))
    k = (1.0 - grid.astype(np.float64)) * 2.0 ** 24
    assert np.array_equal(k, np.round(k))                       # the grid 1 - k 2^-24
    # ... on which the oracle goes from k = 2 (hi, inside) straight to k = 0 (1.0, outside); k = 1 is a float as well, and
    # a device that lands there is outside the clip where the oracle is inside: why no test row sits near the boundary
    assert {0.0, 2.0} <= set(k.tolist()) and 1.0 not in set(k.tolist())


@pytest.mark.parametrize("route", ["mlp", "deepfm", "mlp-uncertainty"])
def test_oracle_clip_gate_matches_float64_autograd(route):
    """oracle/tower.py's hand-written `inside` against autograd of oracle/torch_ref.keras_bce's clamp, in float64, on a mixed
    batch with dropout: the clipped rows carry no gradient on either side, at the bars of
    tests/test_oracle_crosscheck.py::_check_grads.  (In float64 the sigmoid leaves the clip at |z| = 16.12: every row
    saturated in fp32 is clipped there too, every normal row is inside on both sides -- no row sits between the two.)"""
    from oracle import torch_ref as tref
    from test_oracle_crosscheck import _check_grads
    prob = host_problem(route, 0.5)
    _, guess = sat.saturate(prob)
    step, idx, z = sat.pick(prob, sat.MIXED, 0, guess=guess)
    m = prob.model
    uid, pid, dom, label = prob.batch(idx)
    masks = otower.train_masks(m.seed, step, 24, m.hidden, 0.5)
    loss32, g32, _ = prob.loss_and_grads(idx, step)
    names = [n for n in m.names]
    loss64, g64, p64, _ = tref.loss_and_grads(m.params, names, uid, pid, dom, label, masks, 0.5,
                                              route.split("-")[0], m.uncertainty)
    # the loss, row by row: a clipped row's is one of the four fp32 constants (float64 clips at 1 - 1e-7 itself, not at its
    # fp32 neighbour 1 - 2^-23, and has other constants: 16.118 for 15.942), a normal row's is float64's within one ulp of p
    rows32 = otower.bce_per_row(otower.sigmoid(z), label.astype(F32)).astype(np.float64)
    z64, y64 = z.astype(np.float64), label.astype(np.float64)
    rows64 = np.maximum(z64, 0) - z64 * y64 + np.log1p(np.exp(-np.abs(z64)))
    for r in range(24):
        if abs(z64[r]) <= 6:
            assert abs(rows32[r] - rows64[r]) <= 2e-6 * max(1.0, rows64[r]) + 2.0 ** -24 * (1 + np.exp(abs(z64[r]))), r
        else:
            want = {(True, 0): sat.LOSS_HIGH_Y0, (True, 1): sat.LOSS_HIGH_Y1, (False, 1): sat.LOSS_LOW_Y1,
                    (False, 0): sat.LOSS_LOW_Y0}[(bool(z64[r] > 0), int(label[r]))]
            assert abs(rows32[r] - want) <= 5e-3 * want, (r, rows32[r], want)
    assert sorted(g32) == sorted(names)
    # (the uncertainty scalar's gradient -2 mean(BCE) / var^3 + 1 / var carries the clipped rows' constants: held to the
    # formula on the fp32 rows instead)
    _check_grads(g32, g64, [n for n in names if n != "log_var"])
    if m.uncertainty:
        var = float(m.params["log_var"][prob.d])
        np.testing.assert_allclose(g32["log_var"][prob.d], -2 * rows32.mean() / var ** 3 + 1 / var, rtol=1e-5)
        assert not np.any(np.delete(g32["log_var"], prob.d))
    # ... and the gate alone: an all-saturated batch has no data gradient at all, in fp32 as in float64
    step5, idx5, _ = sat.pick(prob, sat.ALL_SATURATED_5, step + 1, guess=guess, exclude=idx)
    uid, pid, dom, label = prob.batch(idx5)
    masks = otower.train_masks(m.seed, step5, 5, m.hidden, 0.5)
    _, g32, _ = prob.loss_and_grads(idx5, step5)
    _, g64, _, _ = tref.loss_and_grads(m.params, names, uid, pid, dom, label, masks, 0.5, route.split("-")[0], m.uncertainty)
    for n in names:
        if n not in ("domain_emb", "lin_domain", "log_var"):
            assert not np.any(g32[n]) and not np.any(g64[n]), n
