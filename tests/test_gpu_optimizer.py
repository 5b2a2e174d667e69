"""Every Adam update site of the library held to a float64 TF1 `ApplyAdam` (oracle/adam64.py) element by element, at the
states where an optimiser goes wrong late in training.

Sites (each reached through its own dispatch):
  IEEE `/` and `sqrtf`, K = 4
    fused_kernels.hip:66-77     fz_opt (k_wgrad_adam)                    dense tower, batch 256 and 1,024 (fused path)
    step_kernels.hip:1466-1474  optimizer_step (k_update on slabs)       MAMDR_FUSED=0 at 256, and batch 4,096
    mamdr_kernels.h:72-76,270-276  dm_apply4 / dm_apply1 (DmStep)        the domain-table row's pending step
    star_kernels.hip:52-66      opt_apply                                the live Star slice
    graph_engine.hip:586-597    opt_elem                                 generic-layer engine, eps 1e-8 and 1e-7
    outer_kernels.hip:185-191   AdamApply (mamdr_adam_apply)             MAML's outer step, grad_scale != 1
  hardware v_sqrt_f32 / v_rcp_f32, K = 7
    emb_bodies.h:29-47          adam_elem / adam_elem_zero               trainable-table rows: touched rows (k_emb_reduce),
                                                                         lagging rows (k_emb_catchup), k_emb_flush,
                                                                         k_emb_sweep (MAMDR_DENSE_ADAM=1), DeepFM's linear
                                                                         tables, the generic engine's tables
    star_kernels.hip:39-44      adam_zero_step                           the non-live Star slices, per step and in
                                                                         k_star_catchup

The gradient a step sees is read from a PROBE: a second context with beta1 = 0 (omb1 = 1), the same weights, batch and
dropout position, whose step writes m = (g - 0) * 1 + 0 = g exactly at every site (gk = g + 2 l2 p at the table sites).
The probe is run twice and its two gradients must be bit-identical.

States (t = optimiser steps already taken; the step under test is t + 1): t = 0 with zero slots; t = 850 (beta1^t
denormal); t = 1,000 (beta1^t at its denormal fixed point 4 x 2^-149 -- with round-to-nearest the fp32 product never
reaches 0); t = 17,000 (1 - beta2^t rounds to 1); t = 200,000 (both products at their fixed points: set_counters stops
early).  The slots are seeded per element: zero, of the gradient's size, sqrt(v) ~ eps (eps dominates the denominator);
elements whose gradient is exactly 0 keep their seeded (m, v), and with m = v = 0 must keep p's bits.
"""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import adam64 as A          # noqa: E402
from oracle import rng as orng          # noqa: E402
from oracle import tower as otower      # noqa: E402

F32 = np.float32
LR = 1e-3
STATES = (0, 850, 1000, 17000, 200000)
REPORT = {}


def _report(site, t, got, exact, exc, denorm):
    r = REPORT.setdefault(site, {"m": 0.0, "v": 0.0, "p": 0.0, "bar": 0.0, "ftz": 0, "denormal_kept": 0})
    for k, (a, b) in zip("pmv", zip(got, exact)):
        r[k] = max(r[k], float(A.ulps(a, b).max()) if a.size else 0.0)
    r["bar"] = max(r["bar"], max(float(e.max()) if e.size else 0.0 for e in exc))
    r["ftz"] += denorm[0]
    r["denormal_kept"] += denorm[1]


def _report_one(site, name, got, exact, exc):
    r = REPORT.setdefault(site, {"m": 0.0, "v": 0.0, "p": 0.0, "bar": 0.0, "ftz": 0, "denormal_kept": 0})
    r[name] = max(r[name], float(A.ulps(got, exact).max()))
    r["bar"] = max(r["bar"], float(exc.max()))


@pytest.fixture(scope="module", autouse=True)
def _print_report():
    yield
    for site, r in sorted(REPORT.items()):
        print("ADAM64 %-34s max ulps m %.2f v %.2f p %.2f | worst error / bar %.3f | denormal results: %d flushed to 0, %d kept"
              % (site, r["m"], r["v"], r["p"], r["bar"], r["ftz"], r["denormal_kept"]))


def check(site, t, g, p0, m0, v0, got, alpha, omb1, omb2, eps=1e-8, hw=None, mask=None):
    """assert (p, m, v) = got against one exact step from (p0, m0, v0) with gradient g, the bars of oracle/adam64.py.
    hw: boolean mask of the elements on a hardware-rcp site; mask: the elements the step covers."""
    p1, m1, v1 = got
    if mask is not None:
        g, p0, m0, v0, p1, m1, v1 = (x[mask] for x in (g, p0, m0, v0, p1, m1, v1))
        hw = None if hw is None else hw[mask]
    hw = np.zeros(g.shape, bool) if hw is None else hw
    (ps, ms, vs), (bp, bm, bv) = A.bars(g, p0, m0, v0, alpha, omb1, omb2, eps, hw=False, m_got=m1, v_got=v1)
    (_, _, _), (bph, _, _) = A.bars(g, p0, m0, v0, alpha, omb1, omb2, eps, hw=True, m_got=m1, v_got=v1)
    bp = np.where(hw, bph, bp)
    exc = [A.excess(p1, ps, bp), A.excess(m1, ms, bm), A.excess(v1, vs, bv)]
    den = [0, 0]
    for got_, ex in ((p1, ps), (m1, ms), (v1, vs)):
        sub = (np.abs(ex) < A.TINY) & (ex != 0)
        den[0] += int((sub & (got_ == 0)).sum())
        den[1] += int((sub & (got_ != 0)).sum())
    _report(site, t, (p1, m1, v1), (ps, ms, vs), exc, den)
    for name, e, a, b in zip("pmv", exc, (p1, m1, v1), (ps, ms, vs)):
        bad = np.flatnonzero(e > 1.0)
        assert bad.size == 0, (site, t, name, bad.size, int(bad[0]), float(a[bad[0]]), float(b[bad[0]]), float(e.max()))
    for x in (p1, m1, v1):
        assert np.isfinite(x).all(), (site, t)
    still = (g == 0) & (m0 == 0) & (v0 == 0)
    assert np.array_equal(p1[still].view(np.uint32), p0[still].view(np.uint32)), (site, t, "p moved at g = m = v = 0")


def seed_slots(g, t, rs, eps=1e-8):
    """per-element (m, v): zero / gradient-sized / sqrt(v) ~ eps, in three interleaved thirds (all zero at t = 0)."""
    n = g.size
    if t == 0:
        return np.zeros(n, F32), np.zeros(n, F32)
    scale = np.abs(g.astype(np.float64))
    scale = np.where(scale > 0, scale, np.median(scale[scale > 0]) if (scale > 0).any() else 1e-3)
    kind = np.arange(n) % 3
    m = rs.standard_normal(n) * scale
    v = np.square(scale * rs.uniform(0.3, 3.0, n))
    v = np.where(kind == 2, np.square(eps * rs.uniform(0.2, 5.0, n)), v)
    m = np.where(kind == 2, rs.standard_normal(n) * eps * 0.1, m)
    m = np.where(kind == 0, 0.0, m)
    v = np.where(kind == 0, 0.0, v)
    return m.astype(F32), v.astype(F32)


def _host(x):
    return x.detach().cpu().numpy().copy()


def run_step(eng, t, ds, p0, m0, v0, train):
    """set_counters FIRST (it flushes lagging rows at the old count and marks every row current), then the state, then
    one step; returns the synchronised (p, m, v)."""
    dev = eng.device
    eng.set_counters(t, ds)
    eng.set_weights(torch.from_numpy(p0).to(dev))
    eng.adam_m.copy_(torch.from_numpy(m0).to(dev))
    eng.adam_v.copy_(torch.from_numpy(v0).to(dev))
    train(eng)
    torch.cuda.synchronize(dev)
    return _host(eng.weights), _host(eng.adam_m), _host(eng.adam_v)


def probe_grad(probe, t, ds, p0, v0, train):
    z = np.zeros_like(p0)
    _, g1, _ = run_step(probe, t, ds, p0, z, v0, train)
    _, g2, _ = run_step(probe, t, ds, p0, z, v0, train)
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32)), "the probe's gradient is not reproducible"
    return g1


# ---------------------------------------------------------------- problems
def _tower_params(g, rs, tower, emb_trainable):
    params = otower.init_params(rs, g["n_user"], g["n_item"], g["n_domain"])
    params["user_emb"], params["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    params["domain_emb"] = (rs.standard_normal(params["domain_emb"].shape) * 0.05).astype(F32)
    for l in range(3):
        params["b%d" % l] = (rs.standard_normal(params["b%d" % l].shape) * 0.05).astype(F32)
    if tower in ("deepfm", "wdl"):
        params["lin_domain"] = (rs.standard_normal(g["n_domain"]) * 0.05).astype(F32)
        if emb_trainable:
            params["lin_user"] = (rs.standard_normal(g["n_user"]) * 0.05).astype(F32)
            params["lin_item"] = (rs.standard_normal(g["n_item"]) * 0.05).astype(F32)
    return params


def make_towers(batch=256, tower="mlp", emb_trainable=False, dropout=0.5, seed=7, scale=0.05, beta2=0.999, data=None):
    """(g, real context, probe context, packed weights); star: the Star tower's parameters (oracle/star.py)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine, synthetic
    g = synthetic.generate("taobao10", batch_size=batch, seed=seed, scale=scale)
    rs = np.random.RandomState(seed)
    if tower == "star":
        from oracle import star as ostar
        params = ostar.init_params(rs, g["n_user"], g["n_item"], g["n_domain"])
        params["user_emb"], params["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
        for n in ("pn_gamma_shared", "pn_gamma_spec"):
            params[n] = (params[n] + rs.standard_normal(params[n].shape) * 0.2).astype(F32)
        for n in ("pn_beta_shared", "pn_beta_spec", "bs0", "bs1", "bs2", "bd0", "bd1", "bd2", "gb"):
            params[n] = (rs.standard_normal(params[n].shape) * 0.05).astype(F32)
    else:
        params = _tower_params(g, rs, tower, emb_trainable)
    engs = []
    for b1 in (0.9, 0.0):
        eng = engine.TowerEngine(g["n_user"], g["n_item"], g["n_domain"], batch, dropout=dropout, emb_trainable=emb_trainable,
                                 tower=tower, adam_beta1=b1, adam_beta2=beta2)
        if not emb_trainable:
            eng.bind_table("user_emb", params["user_emb"])
            eng.bind_table("item_emb", params["item_emb"])
        for d in range(g["n_domain"]):
            c = (data or {}).get(d) or g["data"]["train"][d]
            eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
        engs.append(eng)
    p0 = _host(engs[0].pack(params))
    return g, engs[0], engs[1], p0


def hw_mask(eng, tower, emb_trainable, live=None):
    """elements updated by a hardware-rcp recipe: trainable-table rows (and DeepFM's linear tables); Star: the per-domain
    slices of every domain but `live`."""
    hw = np.zeros(eng.n_params, bool)
    if emb_trainable:
        for name in ("user_emb", "item_emb", "lin_user", "lin_item"):
            if name in eng.segments:
                off, cnt = eng.segments[name]
                hw[off:off + cnt] = True
    if tower == "star" and live is not None:
        for name in ("Wd0", "Wd1", "Wd2", "bd0", "bd1", "bd2", "pn_gamma_spec", "pn_beta_spec"):
            off, cnt = eng.segments[name]
            per = cnt // eng.n_domain
            hw[off:off + cnt] = True
            hw[off + live * per:off + (live + 1) * per] = False
    return hw


def seg_mask(eng):
    """the elements of the flat vector that belong to a tensor (not the alignment padding between them)."""
    mask = np.zeros(eng.n_params, bool)
    for off, cnt in eng.segments.values():
        mask[off:off + cnt] = True
    return mask


def _largest(g, k=1):
    sizes = [g["data"]["train"][d]["uid"].shape[0] for d in range(g["n_domain"])]
    return sorted(range(g["n_domain"]), key=lambda d: -sizes[d])[:k], sizes


def _states_on(site, real, probe, p0, train, hw, ds=3, seed=0, states=STATES, eps=1e-8):
    rs = np.random.RandomState(seed)
    for t in states:
        alpha, omb1, omb2, _, _ = A.scalars(t, LR)
        g = probe_grad(probe, t, ds, p0, np.zeros_like(p0), train)
        assert np.abs(g).max() > 0
        m0, v0 = seed_slots(g, t, rs, eps)
        got = run_step(real, t, ds, p0, m0, v0, train)
        check(site, t, g, p0, m0, v0, got, alpha, omb1, omb2, eps, hw=hw, mask=seg_mask(real))


# ---------------------------------------------------------------- dense towers and the domain-table row
@pytest.mark.parametrize("path,batch,mixed", [("k_wgrad_adam", 256, False), ("k_wgrad_adam", 1024, False),
                                              ("k_wgrad_adam", 1024, True), ("k_update", 256, False),
                                              ("k_update", 4096, False)])
def test_dense_tower_and_domain_row(path, batch, mixed):
    """the MLP tower over frozen tables: every dense weight (fz_opt or optimizer_step) and the domain table (the pending
    DmStep, on one-domain batches or on a batch whose domain column mixes four ids), one step at every state."""
    env = {"MAMDR_FUSED": "0"} if (path == "k_update" and batch <= 1024) else {}
    os.environ.update(env)
    try:
        g, real, probe, p0 = make_towers(batch=batch)
        (d,), sizes = _largest(g)
        if batch > sizes[d]:          # one batch of every domain's rows (the domain column mixes all ten ids)
            cols = {k: np.concatenate([g["data"]["train"][j][k] for j in range(g["n_domain"])]) for k in ("uid", "pid", "domain", "label")}
            sizes[d] = cols["uid"].shape[0]
            assert sizes[d] >= batch
            for e in (real, probe):
                e.bind_domain_data(d, "train", cols["uid"], cols["pid"], cols["domain"], cols["label"])
        if mixed:
            cols = {k: v.copy() for k, v in g["data"]["train"][d].items()}
            cols["domain"][:] = np.random.RandomState(3).choice([1, 4, 7, 9], size=sizes[d]).astype(cols["domain"].dtype)
            for e in (real, probe):
                e.bind_domain_data(d, "train", cols["uid"], cols["pid"], cols["domain"], cols["label"])
        want = "k_wgrad_adam" if path == "k_wgrad_adam" else "k_wgrad"
        from mamdr_amd import _lib as L
        assert real.step_kernel_names(batch)[L.KERNEL_WGRAD] == want
        perm = torch.from_numpy(orng.shuffle_perm(sizes[d], 10000, seed=5)).to(real.device)

        def train(e):
            e.train_steps(d, perm=perm, first_step=0, n_steps=1, lr=LR)
        _states_on("%s b%d%s" % (path, batch, " mixed" if mixed else ""), real, probe, p0, train, None)
    finally:
        for k in env:
            os.environ.pop(k, None)
    real.close()
    probe.close()


# ---------------------------------------------------------------- trainable tables
@pytest.mark.parametrize("tower,dense", [("mlp", False), ("mlp", True), ("deepfm", False)])
def test_trainable_table_rows(tower, dense):
    """tables in the flat vector: touched rows (rows repeated inside the batch), the untouched rows' step through the
    flush on the weight read (lazy) or the per-step sweep (MAMDR_DENSE_ADAM=1), DeepFM's linear tables."""
    env = {"MAMDR_DENSE_ADAM": "1"} if dense else {}
    os.environ.update(env)
    try:
        g, real, probe, p0 = make_towers(batch=256, tower=tower, emb_trainable=True)
    finally:
        for k in env:
            os.environ.pop(k, None)
    (d,), sizes = _largest(g)
    perm_h = orng.shuffle_perm(sizes[d], 10000, seed=9)
    assert len(np.unique(g["data"]["train"][d]["uid"][perm_h[:256]])) < 256       # duplicates in the batch
    perm = torch.from_numpy(perm_h).to(real.device)

    def train(e):
        e.train_steps(d, perm=perm, first_step=0, n_steps=1, lr=LR)
    _states_on("tables %s %s" % (tower, "sweep" if dense else "lazy"), real, probe, p0, train,
               hw_mask(real, tower, True), states=(0, 1000, 200000))
    real.close()
    probe.close()


@pytest.mark.parametrize("cap", [None, 8])
def test_lazy_row_caught_up_across_the_beta1_underflow(cap):
    """set_counters(980), 40 steps that do not touch a user row and an item row, then a batch that does: the lagging
    rows' 40 replayed steps (gradient 2 l2 p alone) against adam64.replay -- read once through the flush, once through
    k_emb_catchup in front of the touching step -- and the touching step itself against one exact step.  cap 8: the
    alpha ring wraps (MAMDR_LAZY_LOG_CAP)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import synthetic
    g0 = synthetic.generate("taobao10", batch_size=256, seed=7, scale=0.05)
    cols = {k: v.copy() for k, v in g0["data"]["train"][0].items()}
    n_rows = 41 * 256
    rs = np.random.RandomState(1)
    r_u, r_i = 5, 7
    uid = rs.randint(0, g0["n_user"], n_rows).astype(np.int32)
    pid = rs.randint(0, g0["n_item"], n_rows).astype(np.int32)
    uid[uid == r_u] = r_u + 1
    pid[pid == r_i] = r_i + 1
    uid[40 * 256 + 3], uid[40 * 256 + 90] = r_u, r_u          # the touching batch holds row r_u twice
    pid[40 * 256 + 17] = r_i
    data = {0: {"uid": uid, "pid": pid, "domain": np.zeros(n_rows, np.int32),
                "label": (rs.uniform(size=n_rows) < 0.3).astype(F32)}}
    del cols
    env = {"MAMDR_LAZY_LOG_CAP": str(cap)} if cap else {}
    os.environ.update(env)
    try:
        ctxs = [make_towers(batch=256, emb_trainable=True, data=data) for _ in range(2)]
    finally:
        for k in env:
            os.environ.pop(k, None)
    g, r1, probe, p0 = ctxs[0]
    _, r2, probe2, _ = ctxs[1]
    probe2.close()
    t0, L_ = 980, 40
    rs = np.random.RandomState(2)
    alpha0, omb1, omb2, _, _ = A.scalars(t0, LR)
    gr = probe_grad(probe, t0, 0, p0, np.zeros_like(p0), lambda e: e.train_steps(0, first_step=0, n_steps=1, lr=LR))
    m0, v0 = seed_slots(gr, 1, rs)
    two_l2 = float(F32(2.0) * F32(1e-5))
    alphas = [A.scalars(t, LR)[0] for t in range(t0, t0 + L_)]
    rows = []
    for name, r in (("user_emb", r_u), ("item_emb", r_i)):
        off = r1.segments[name][0]
        rows.append(np.arange(off + r * 128, off + (r + 1) * 128))
    rows = np.concatenate(rows)
    s40 = run_step(r1, t0, 0, p0, m0, v0, lambda e: e.train_steps(0, first_step=0, n_steps=L_, lr=LR))
    rp, rm, rv, (bp, bm, bv) = A.replay(p0[rows], m0[rows], v0[rows], alphas, omb1, omb2, two_l2=two_l2)
    for name, got, want, bar in (("p", s40[0], rp, bp), ("m", s40[1], rm, bm), ("v", s40[2], rv, bv)):
        e = A.excess(got[rows], want, bar)
        _report_one("lazy replay 40 (flush)%s" % (" ring8" if cap else ""), name, got[rows], want, e)
        assert e.max() <= 1.0, (name, float(e.max()))
    s41 = run_step(r2, t0, 0, p0, m0, v0, lambda e: e.train_steps(0, first_step=0, n_steps=L_ + 1, lr=LR))
    t1 = t0 + L_
    alpha1, _, _, _, _ = A.scalars(t1, LR)
    gk = probe_grad(probe, t1, L_, s40[0], np.zeros_like(p0), lambda e: e.train_steps(0, first_step=L_, n_steps=1, lr=LR))
    assert gk[rows].any()
    check("lazy catch-up + touch%s" % (" ring8" if cap else ""), t1, gk, s40[0], s40[1], s40[2], s41, alpha1, omb1, omb2,
          hw=hw_mask(r2, "mlp", True), mask=seg_mask(r2))
    for e in (r1, r2, probe):
        e.close()


# ---------------------------------------------------------------- Star
def test_star_live_and_non_live_slices():
    """Star tower: the live slice (opt_apply) and the other domains' slices (adam_zero_step) swept in a one-step call at
    every state; then a call of 40 steps from t = 980 whose absent domains' slices are replayed by k_star_catchup
    across the beta1 underflow, against adam64.replay."""
    g, real, probe, p0 = make_towers(batch=256, tower="star", dropout=0.0, seed=11)
    (d,), sizes = _largest(g)
    perm = torch.from_numpy(orng.shuffle_perm(sizes[d], 10000, seed=5)).to(real.device)
    hw = hw_mask(real, "star", False, live=d)

    def train(e):
        e.train_steps(d, perm=perm, first_step=0, n_steps=1, lr=LR)
    _states_on("star one-step", real, probe, p0, train, hw)
    # k_star_catchup: the non-live slices see zero gradients over a 40-step call
    gz = probe_grad(probe, 980, 0, p0, np.zeros_like(p0), train)
    assert not gz[hw].any()
    n = min(40, -(-sizes[d] // 256))
    rs = np.random.RandomState(4)
    m0, v0 = seed_slots(np.where(hw, 1e-3, gz).astype(F32), 1, rs)
    got = run_step(real, 980, 0, p0, m0, v0, lambda e: e.train_steps(d, perm=perm, first_step=0, n_steps=n, lr=LR))
    alphas = [A.scalars(t, LR)[0] for t in range(980, 980 + n)]
    _, omb1, omb2, _, _ = A.scalars(980, LR)
    rp, rm, rv, (bp, bm, bv) = A.replay(p0[hw], m0[hw], v0[hw], alphas, omb1, omb2)
    for name, x, want, bar in (("p", got[0], rp, bp), ("m", got[1], rm, bm), ("v", got[2], rv, bv)):
        e = A.excess(x[hw], want, bar)
        _report_one("star k_star_catchup %d" % n, name, x[hw], want, e)
        assert e.max() <= 1.0, (name, float(e.max()))
    real.close()
    probe.close()


# ---------------------------------------------------------------- generic-layer engine
@pytest.mark.parametrize("eps", [1e-8, 1e-7])
def test_graph_engine(eps):
    """the generic-layer engine (opt_elem) with trainable tables (adam_elem), shared bottom, eps 1e-8 and after
    set_adam_eps(1e-7); a step on domain d covers the tables, the shared range and d's task block."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import graph_engine, synthetic
    from oracle import mtl as omtl
    shape = dict(synthetic.SHAPES["taobao10"], n_domain=4)
    g = synthetic.generate(shape, batch_size=256, seed=7, scale=0.05)
    spec = omtl.Spec("shared_bottom", 4, (256, 128), (64,), ())
    rs = np.random.RandomState(7)
    params = omtl.init_params(rs, spec, g["n_user"], g["n_item"])
    params["user_emb"], params["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    for n in params:
        if "/b" in n or n.endswith("/gb") or n == "domain_emb":
            params[n] = (rs.standard_normal(params[n].shape) * 0.05).astype(F32)
    engs = []
    for b1 in (0.9, 0.0):
        e = graph_engine.GraphEngine("shared_bottom", g["n_user"], g["n_item"], 4, 256, (256, 128), (64,), (),
                                     dropout=0.5, emb_trainable=True, adam_beta1=b1)
        for dd in range(4):
            c = g["data"]["train"][dd]
            e.bind_domain_data(dd, "train", c["uid"], c["pid"], c["domain"], c["label"])
        if eps != 1e-8:
            e.set_adam_eps(eps)
        engs.append(e)
    real, probe = engs
    p0 = _host(real.pack(params))
    d = max(range(4), key=lambda k: g["data"]["train"][k]["uid"].shape[0])
    perm = torch.from_numpy(orng.shuffle_perm(g["data"]["train"][d]["uid"].shape[0], 10000, seed=3)).to(real.device)
    mask = np.zeros(real.n_params, bool)
    hw = np.zeros(real.n_params, bool)
    for name in ("user_emb", "item_emb"):
        off, cnt = real.segments[name]
        mask[off:off + cnt] = hw[off:off + cnt] = True
    for off, cnt in real.task_ranges(d):
        mask[off:off + cnt] = True
    mask &= seg_mask(real)

    def train(e):
        e.train_steps(d, perm=perm, first_step=0, n_steps=1, lr=LR)
    rs = np.random.RandomState(1)
    for t in (0, 1000, 17000, 200000):
        alpha, omb1, omb2, _, _ = A.scalars(t, LR)
        gg = probe_grad(probe, t, 2, p0, np.zeros_like(p0), train)
        m0, v0 = seed_slots(gg, t, rs, eps)
        got = run_step(real, t, 2, p0, m0, v0, train)
        check("graph shared_bottom eps %g" % eps, t, gg, p0, m0, v0, got, alpha, omb1, omb2, F32(eps), hw=hw, mask=mask)
        out = seg_mask(real) & ~mask
        for x, x0 in zip(got, (p0, m0, v0)):           # the variables outside the step's model: bit-unchanged
            assert np.array_equal(x[out].view(np.uint32), x0[out].view(np.uint32))
    real.close()
    probe.close()


# ---------------------------------------------------------------- MAML's outer step
def test_outer_adam_apply():
    """mamdr_adam_apply (AdamApply) with grad_scale 0.25 at every state, on a length that is no multiple of 4."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine
    eng = engine.TowerEngine(200, 200, 2, 256, dropout=0.0)
    rs = np.random.RandomState(5)
    n = 100003
    for t in STATES:
        alpha, omb1, omb2, b1p, b2p = A.scalars(t, LR)
        g = (rs.standard_normal(n) * 1e-2).astype(F32)
        g[::17] = 0
        gs = (g * F32(0.25)).astype(F32)
        p0 = (rs.standard_normal(n) * 0.05).astype(F32)
        m0, v0 = seed_slots(gs, t, rs)
        p, m, v, gd = (torch.from_numpy(x.copy()).to(eng.device) for x in (p0, m0, v0, g))
        eng.adam_apply(p, m, v, gd, LR, float(b1p), float(b2p), grad_scale=0.25)
        torch.cuda.synchronize()
        check("mamdr_adam_apply gscale 0.25", t, gs, p0, m0, v0, (_host(p), _host(m), _host(v)), alpha, omb1, omb2)
    eng.close()


# ---------------------------------------------------------------- the beta-power loop
@pytest.mark.parametrize("which", ["tower", "graph"])
def test_set_counters_with_beta2_one_returns_at_once(which):
    """beta2 = 1 keeps its running product at 1: set_counters(0x7ffffff0) must stop once neither product changes (not
    after 2^31 host iterations).  The next step has alpha = 0: p bit-unchanged, m and v updated as adam64 says."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import graph_engine, synthetic
    if which == "tower":
        g, real, probe, p0 = make_towers(batch=256, beta2=1.0)
        probe.close()
    else:
        shape = dict(synthetic.SHAPES["taobao10"], n_domain=2)
        g = synthetic.generate(shape, batch_size=256, seed=7, scale=0.05)
        real = graph_engine.GraphEngine("shared_bottom", g["n_user"], g["n_item"], 2, 256, (128,), (64,), (),
                                        dropout=0.0, emb_trainable=False, adam_beta2=1.0)
        real.bind_table("user_emb", g["tables"]["user_emb"])
        real.bind_table("item_emb", g["tables"]["item_emb"])
        for dd in range(2):
            c = g["data"]["train"][dd]
            real.bind_domain_data(dd, "train", c["uid"], c["pid"], c["domain"], c["label"])
        p0 = (np.random.RandomState(3).standard_normal(real.n_params) * 0.05).astype(F32)
    t0 = time.perf_counter()
    real.set_counters(0x7ffffff0, 0)
    assert time.perf_counter() - t0 < 0.5
    real.set_weights(torch.from_numpy(p0).to(real.device))
    real.adam_m.zero_()
    real.adam_v.zero_()
    real.train_steps(0, first_step=0, n_steps=1, lr=LR)
    torch.cuda.synchronize()
    p, m, v = _host(real.weights), _host(real.adam_m), _host(real.adam_v)
    assert np.array_equal(p.view(np.uint32), p0.view(np.uint32))
    assert np.abs(m).max() > 0 and np.isfinite(m).all() and np.isfinite(v).all()
    alpha, omb1, omb2, _, b2p = A.scalars(0x7ffffff0, LR, beta2=1.0)
    assert alpha == 0 and b2p == 1
    real.close()
