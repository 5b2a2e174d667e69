"""The power of oracle/adam64.py's bars (CPU): the semantic slips an Adam site could make -- each built as a variant of the
float64 reference -- must break the bar by >= 4x on at least 1 % of the elements the slip touches, on the seeded states
and the state schedule of tests/test_gpu_optimizer.py, with gradients of the oracle tower (oracle/tower.py) for a batch
of the size the kernels see.  And adam64 itself against the fp32 TF1 Adam of oracle/tower.py and oracle/mtl.py.
"""
import numpy as np
import pytest

from oracle import adam64 as A
from oracle import tower as otower

F32 = np.float32
LR = 1e-3
STATES = (0, 850, 1000, 17000, 200000)
TWO_L2 = float(F32(2.0) * F32(1e-5))


def seed_slots(g, t, rs, eps=1e-8):
    """as tests/test_gpu_optimizer.py: zero / gradient-sized / sqrt(v) ~ eps thirds, all zero at t = 0."""
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


@pytest.fixture(scope="module")
def problem():
    """an MLP tower with trainable tables, one batch of 256 rows: the raw gradient (no regulariser) of every element,
    the parameters and which table rows the batch touches."""
    rs = np.random.RandomState(0)
    n_user, n_item, n_domain = 400, 300, 4
    params = otower.init_params(rs, n_user, n_item, n_domain)
    params["user_emb"] = rs.uniform(-0.05, 0.05, params["user_emb"].shape).astype(F32)
    params["item_emb"] = rs.uniform(-0.05, 0.05, params["item_emb"].shape).astype(F32)
    params["domain_emb"] = (rs.standard_normal(params["domain_emb"].shape) * 0.05).astype(F32)
    for l in range(3):
        params["b%d" % l] = (rs.standard_normal(params["b%d" % l].shape) * 0.05).astype(F32)
    B = 256
    uid = rs.randint(0, n_user, B).astype(np.int32)
    pid = rs.randint(0, n_item, B).astype(np.int32)
    dom = np.full(B, 1, np.int32)
    y = (rs.rand(B) < 0.3).astype(F32)
    masks = otower.train_masks(1024, 0, B, (256, 128, 64), 0.5)
    _, grads, _ = otower.loss_and_grads(params, uid, pid, dom, y, masks, 0.5, True, l2=(0.0, 0.0))
    names = otower.param_names(True)
    g = np.concatenate([np.asarray(grads[n], F32).ravel() for n in names])
    p = np.concatenate([np.asarray(params[n], F32).ravel() for n in names])
    table = np.zeros(g.size, bool)
    touched = np.zeros(g.size, bool)
    off = 0
    for n in names:
        cnt = params[n].size
        if n in ("user_emb", "item_emb"):
            table[off:off + cnt] = True
            ids = np.unique(uid if n == "user_emb" else pid)
            rows = (off + ids[:, None] * 128 + np.arange(128)[None, :]).ravel()
            touched[rows] = True
        off += cnt
    assert 0 < touched.sum() < table.sum()
    # the kernels' table gradient: gk = fl(fl(2 l2 p) + g) on every row
    gk = np.where(table, ((F32(TWO_L2) * p).astype(F32) + g).astype(F32), g).astype(F32)
    return dict(g=g, gk=gk, p=p, table=table, touched=touched)


def _fp32_step(g, p, m, v, alpha, omb1, omb2, eps, keras=False, b1=None, b2=None):
    """an fp32 site: TF's slot form (or Keras' beta m + (1 - beta) g), IEEE divide."""
    if keras:
        m1 = (F32(b1) * m + (omb1 * g).astype(F32)).astype(F32)
        v1 = (F32(b2) * v + (omb2 * (g * g).astype(F32)).astype(F32)).astype(F32)
    else:
        m1 = (m + ((g - m).astype(F32) * omb1).astype(F32)).astype(F32)
        v1 = (v + (((g * g).astype(F32) - v).astype(F32) * omb2).astype(F32)).astype(F32)
    d = ((m1 * alpha).astype(F32) / (np.sqrt(v1, dtype=F32) + F32(eps)).astype(F32)).astype(F32)
    return (p - d).astype(F32), m1, v1


def _excess(g, p, m, v, t, got, which="any", eps=1e-8, mask=None):
    """got / bar of p, m or v -- or, "any", the largest of the three (a site is held to all three bars at once)."""
    alpha, omb1, omb2, _, _ = A.scalars(t, LR)
    (ps, ms, vs), (bp, bm, bv) = A.bars(g, p, m, v, alpha, omb1, omb2, eps, m_got=got[1], v_got=got[2])
    e = {"p": A.excess(got[0], ps, bp), "m": A.excess(got[1], ms, bm), "v": A.excess(got[2], vs, bv)}
    e = np.maximum(np.maximum(e["p"], e["m"]), e["v"]) if which == "any" else e[which]
    return e if mask is None else e[mask]


def _schedule(problem, slip, which="any", states=STATES):
    """the fraction of the touched elements that the slip puts >= 4x beyond the bar, over the state schedule."""
    rs = np.random.RandomState(3)
    hits, total = 0, 0
    for t in states:
        g, p = problem["gk"], problem["p"]
        m, v = seed_slots(g, t, rs)
        got, touched = slip(g, p, m, v, t)
        if touched is None or not touched.any():
            continue
        e = _excess(g, p, m, v, t, got, which, mask=touched)
        hits += int((e >= 4.0).sum())
        total += int(touched.sum())
    assert total > 0
    return hits / total


def _rejected(frac):
    """a slip is rejected: >= 4x beyond the bar on at least 1 % of the elements it touches."""
    import inspect
    print("%s: %.4f of the touched elements >= 4x the bar" % (inspect.stack()[1].function, frac))
    assert frac >= 0.01


def _scal(t):
    alpha, omb1, omb2, b1p, b2p = A.scalars(t, LR)
    return alpha, omb1, omb2


def test_the_exact_fp32_recipe_passes_its_own_bar(problem):
    """the TF1 fp32 form (IEEE) stays inside the bar at every state: the bar is not simply too tight."""
    rs = np.random.RandomState(3)
    for t in STATES:
        g, p = problem["gk"], problem["p"]
        m, v = seed_slots(g, t, rs)
        alpha, omb1, omb2 = _scal(t)
        got = _fp32_step(g, p, m, v, alpha, omb1, omb2, 1e-8)
        for which in "pmv":
            assert _excess(g, p, m, v, t, got, which).max() <= 1.0, (t, which)


def test_slip_eps_1e7_instead_of_1e8(problem):
    def slip(g, p, m, v, t):
        alpha, omb1, omb2 = _scal(t)
        return _fp32_step(g, p, m, v, alpha, omb1, omb2, 1e-7), np.ones(g.size, bool)
    _rejected(_schedule(problem, slip))


def test_slip_eps_1e8_where_1e7_is_configured(problem):
    """the reverse (the generic engine's DeepMTLCTR init_parms stage runs with eps 1e-7)."""
    rs = np.random.RandomState(3)
    hits = total = 0
    for t in STATES:
        g, p = problem["gk"], problem["p"]
        m, v = seed_slots(g, t, rs, eps=1e-7)
        alpha, omb1, omb2 = _scal(t)
        got = _fp32_step(g, p, m, v, alpha, omb1, omb2, 1e-8)
        e = _excess(g, p, m, v, t, got, eps=F32(1e-7))
        hits += int((e >= 4).sum())
        total += e.size
    _rejected(hits / total)


def test_slip_eps_inside_the_bias_correction(problem):
    """torch's form: p -= lr m_hat / (sqrt(v_hat) + eps), m_hat = m / (1 - b1^t), v_hat = v / (1 - b2^t)."""
    def slip(g, p, m, v, t):
        _, omb1, omb2, b1p, b2p = A.scalars(t, LR)
        m1 = (m + ((g - m) * omb1).astype(F32)).astype(F32)
        v1 = (v + ((g * g - v) * omb2).astype(F32)).astype(F32)
        mh = (m1 / (F32(1) - b1p)).astype(F32)
        vh = (v1 / (F32(1) - b2p)).astype(F32)
        d = ((F32(LR) * mh).astype(F32) / (np.sqrt(vh, dtype=F32) + F32(1e-8))).astype(F32)
        return ((p - d).astype(F32), m1, v1), np.ones(g.size, bool)
    _rejected(_schedule(problem, slip))


def test_slip_beta_powers_by_pow_is_below_the_bar(problem):
    """beta^t by pow() instead of TF's running fp32 product.  NOT rejected, and this test says why: at the schedule's
    states the two alphas are equal or one ulp apart (relative 8e-8 at most), and |delta| << |p| puts that under the
    parameter's own half-ulp rounding.  (The difference peaks near t = 5 at 5e-6 relative -- still under ulp(p) for
    parameters 100x larger than their step.)  The fraction the bar would flag is printed."""
    worst = 0.0
    for t in STATES:
        a = A.scalars(t, LR)[0]
        b1 = F32(np.power(np.float64(F32(0.9)), t + 1))
        b2 = F32(np.power(np.float64(F32(0.999)), t + 1))
        worst = max(worst, abs(float(A.alpha_of(LR, b1, b2)) - float(a)) / float(a))
    assert worst <= 2.0 ** -23

    def slip(g, p, m, v, t):
        _, omb1, omb2, _, _ = A.scalars(t, LR)
        b1 = F32(np.power(np.float64(F32(0.9)), t + 1))
        b2 = F32(np.power(np.float64(F32(0.999)), t + 1))
        return _fp32_step(g, p, m, v, A.alpha_of(LR, b1, b2), omb1, omb2, 1e-8), np.ones(g.size, bool)
    print("pow() beta powers: largest relative alpha difference %.3g, fraction >= 4x the bar %.4f"
          % (worst, _schedule(problem, slip)))


def test_slip_table_regulariser_dropped(problem):
    """the tables' 2 l2 p term left out of the gradient (every table row)."""
    def slip(g, p, m, v, t):
        alpha, omb1, omb2 = _scal(t)
        return _fp32_step(problem["g"], p, m, v, alpha, omb1, omb2, 1e-8), problem["table"]
    _rejected(_schedule(problem, slip))


def test_slip_untouched_rows_not_stepped(problem):
    """torch SparseAdam's semantics: rows the batch does not touch keep p, m, v (TF1 moves every row every step)."""
    def slip(g, p, m, v, t):
        alpha, omb1, omb2 = _scal(t)
        p1, m1, v1 = _fp32_step(g, p, m, v, alpha, omb1, omb2, 1e-8)
        keep = problem["table"] & ~problem["touched"]
        return (np.where(keep, p, p1), np.where(keep, m, m1), np.where(keep, v, v1)), keep
    _rejected(_schedule(problem, slip))


def test_slip_closed_form_decay_over_a_lag():
    """a lagging row brought up L steps at once -- m beta1^L, v beta2^L in one multiply, p moved by L alpha_last m_L /
    (sqrt(v_L) + eps) -- instead of L per-step replays (adam64.replay, the state of the lazy test: t = 980, L = 40)."""
    rs = np.random.RandomState(5)
    n = 20000
    p = (rs.standard_normal(n) * 0.05).astype(F32)
    m = (rs.standard_normal(n) * 1e-4).astype(F32)
    v = np.square(rs.standard_normal(n) * 1e-4).astype(F32)
    L = 40
    alphas = [A.scalars(t, LR)[0] for t in range(980, 980 + L)]
    _, omb1, omb2, _, _ = A.scalars(980, LR)
    rp, rm, rv, (bp, bm, bv) = A.replay(p, m, v, alphas, omb1, omb2, two_l2=TWO_L2)
    mL = (m * F32(0.9 ** L)).astype(F32)
    vL = (v * F32(0.999 ** L)).astype(F32)
    pL = (p - (F32(L) * alphas[-1] * mL / (np.sqrt(vL) + F32(1e-8))).astype(F32)).astype(F32)
    e = np.maximum(A.excess(pL, rp, bp), A.excess(mL, rm, bm))
    _rejected(float(np.mean(e >= 4)))


def test_keras_slot_form_is_reported():
    """Keras' beta m + (1 - beta) g differs from TF's m + (g - m)(1 - beta) by about an ulp: reported, not asserted."""
    rs = np.random.RandomState(9)
    n = 100000
    g = (rs.standard_normal(n) * 1e-3).astype(F32)
    p = (rs.standard_normal(n) * 0.05).astype(F32)
    m, v = seed_slots(g, 1, rs)
    fr = []
    for t in STATES[1:]:
        alpha, omb1, omb2 = _scal(t)
        got = _fp32_step(g, p, m, v, alpha, omb1, omb2, 1e-8, keras=True, b1=0.9, b2=0.999)
        e = _excess(g, p, m, v, t, got, "m")
        fr.append((float(np.mean(e > 1)), float(np.mean(e >= 4))))
    print("keras slot form: fraction of m beyond the bar / >= 4x the bar per state:", fr)


def test_replay_of_zero_steps_is_the_input():
    p, m, v = (np.arange(1, 9, dtype=F32) * s for s in (0.1, 1e-3, 1e-6))
    rp, rm, rv, _ = A.replay(p, m, v, [], F32(0.1), F32(0.001))
    assert np.array_equal(rp, p) and np.array_equal(rm, m) and np.array_equal(rv, v)


def test_adam64_against_the_oracles_fp32_adam():
    """oracle/tower.py's OuterAdam (the fp32 TF1 form) and oracle/mtl.py's per-model Adam within an ulp of adam64 on
    random states (a few ulps where the increment cancels, as the bar allows)."""
    rs = np.random.RandomState(11)
    n = 50000
    for steps in (1, 3, 12):
        opt = otower.OuterAdam(n)
        theta = (rs.standard_normal(n) * 0.05).astype(F32)
        for k in range(steps):
            grad = (rs.standard_normal(n) * 1e-2).astype(F32)
            p0, m0, v0 = theta.copy(), opt.m.copy(), opt.v.copy()
            opt.apply(theta, grad, LR)
            alpha, omb1, omb2, _, _ = A.scalars(k, LR)
            (ps, ms, vs), (bp, bm, bv) = A.bars(grad, p0, m0, v0, alpha, omb1, omb2, m_got=opt.m, v_got=opt.v)
            for got, ex, bar in ((theta, ps, bp), (opt.m, ms, bm), (opt.v, vs, bv)):
                assert A.excess(got, ex, bar).max() <= 1.0
                assert np.median(A.ulps(got, ex)) <= 1.0
    # oracle/mtl.py's per-model Adam (OracleMTL.train_on_batch), fed random gradients in place of a batch's
    from oracle import mtl as omtl
    spec = omtl.Spec("shared_bottom", 2, (64,), (32,), ())
    params = omtl.init_params(np.random.RandomState(1), spec, 30, 20)
    model = omtl.OracleMTL({k: v.copy() for k, v in params.items()}, spec, dropout=0.0, lr=LR)
    real = omtl.loss_and_grads
    try:
        for k in range(3):
            grads = {n: (rs.standard_normal(model.params[n].shape) * 1e-2).astype(F32) for n in model.names}
            omtl.loss_and_grads = lambda *a, **kw: (F32(0), grads, None)
            before = {n: (model.params[n].copy(), model.m[n].copy(), model.v[n].copy()) for n in model.names}
            z = np.zeros(4, np.int32)
            model.train_on_batch(0, z, z, z, np.zeros(4, F32))
            alpha, omb1, omb2, _, _ = A.scalars(k, LR)
            for n in model.names:
                p0, m0, v0 = before[n]
                (ps, ms, vs), (bp, bm, bv) = A.bars(grads[n], p0, m0, v0, alpha, omb1, omb2, m_got=model.m[n],
                                                    v_got=model.v[n])
                for got, ex, bar in ((model.params[n], ps, bp), (model.m[n], ms, bm), (model.v[n], vs, bv)):
                    assert A.excess(got, ex, bar).max() <= 1.0, n
    finally:
        omtl.loss_and_grads = real
