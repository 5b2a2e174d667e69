"""TF1 `ApplyAdam` in float64 on fp32 inputs: the reference every Adam update site of the library is held to, element by
element (tests/test_gpu_optimizer.py), with the bar that says how far a site may be from it.

Host scalars.  The library forms them on the host in fp32, one rounding per operation, and so does `scalars` here:
    omb   = fl(1 - beta)                                    (mamdr_api.hip, graph_engine.hip: omb1 / omb2)
    b1p_t = fl(b1p_{t-1} * beta1), b2p_t likewise           (TF's running beta1_power / beta2_power variables)
    alpha = fl(fl(lr * fl(sqrt(fl(1 - b2p)))) / fl(1 - b1p))  (mamdr_api.hip `adam_alpha`, graph_engine.hip `alpha`,
                                                            mamdr_adam_apply in step_stateless.hip)
Everything after that is evaluated exactly (float64; the few products lose nothing that matters at the bar):
    m* = m + (g - m) omb1,   v* = v + (g^2 - v) omb2,   p* = p - delta*,   delta* = m* alpha / (sqrt(v*) + eps)

Rounding sequences of the sites and the bars they imply (u = 2^-24, first order in u):

  slots, every site:  m = fl(m + fl(fl(g - m) omb1))  (or one fma for the last two roundings)
        |m - m*| <= 0.5 ulp(m*) + 2 u |g - m| omb1
  the subtraction's and the product's roundings act on the increment, not on m*; where g ~ -m beta / (1 - beta) m* cancels
  and the increment term is what is left.  v = fl(v + fl(fl(fl(g g) - v) omb2)) adds the rounding of g g:
        |v - v*| <= 0.5 ulp(v*) + 3 u (g^2 + |v|) omb2
  (hardware-rcp sites form m, v with one fma: fewer roundings, same bar.)

  parameter, IEEE sites (opt_step -- k_wgrad_adam, k_update, AdamApply --, dm_apply, opt_apply, opt_elem):
        delta = fl(fl(m alpha) / fl(fl(sqrt v) + eps))  -- four roundings of relative size <= u: K = 4
  (the issue that introduced this module proposed K = 3; the addition of eps is a fourth rounding, and its error is not
  absorbed by any other: a delta with the three others exact but fl(s + eps) off by half an ulp sits 1 u out.)
  parameter, hardware sites (adam_elem, adam_elem_zero, adam_zero_step):
        delta = fl(fl(m alpha) * rcp(fl(sqrt_hw(v) + eps)))  -- v_sqrt_f32 and v_rcp_f32 are 1 ulp (<= 2u relative
        each), the product, the addition and the final multiply u each: K = 7
  then p = fl(p - delta): half an ulp of the result, taken at the larger of the two floats around p* (a result that
  crosses a power of two rounds on the coarser grid).  The slots the site itself wrote feed delta; their own error (held
  to the slot bars above) is carried into the parameter bar exactly:
        |p - p*| <= 0.5 ulp(p*) + K u |delta*| + alpha |m_got - m*| / (sqrt(v*) + eps) + |delta*| |v_got - v*| / (2 v*)

  Results below 2^-126 (denormal fp32): the IEEE value or 0 (flush-to-zero of the operation that produced it).

`replay` runs L steps with zero gradient (the catch-up of a row no batch touched, the Star slices of absent domains)
with per-step alphas along the exact trajectory, and bounds a site that rounds every step: each step's own bar, plus
the slot errors of the earlier steps (decayed by beta) carried into the later steps' deltas.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
K_IEEE = 4
K_HW = 7
TINY = 2.0 ** -126


def scalars(t, lr=1e-3, beta1=0.9, beta2=0.999):
    """(alpha, omb1, omb2, b1p, b2p) of the optimiser's step t + 1 after t steps, in fp32 as the host forms them."""
    b1 = F32(beta1)
    b2 = F32(beta2)
    b1p, b2p = F32(1), F32(1)
    for _ in range(int(t) + 1):
        nb1, nb2 = F32(b1p * b1), F32(b2p * b2)
        if nb1 == b1p and nb2 == b2p:
            break
        b1p, b2p = nb1, nb2
    return alpha_of(lr, b1p, b2p), F32(F32(1) - b1), F32(F32(1) - b2), b1p, b2p


def alpha_of(lr, b1p, b2p):
    return F32(F32(F32(lr) * F32(np.sqrt(F32(F32(1) - F32(b2p)), dtype=F32))) / F32(F32(1) - F32(b1p)))


def step(g, p, m, v, alpha, omb1, omb2, eps=1e-8, two_l2=0.0):
    """one exact step from fp32 inputs: (p*, m*, v*, delta*) in float64.  two_l2: the tables' regulariser term, formed
    as the kernels form it (gk = fl(fl(two_l2 p) + g)) before the exact part."""
    g = np.asarray(g, F32)
    p = np.asarray(p, F32)
    if two_l2:
        g = (F32(two_l2) * p).astype(F32) + g
        g = g.astype(F32)
    g, p = g.astype(np.float64), p.astype(np.float64)
    m = np.asarray(m, F32).astype(np.float64)
    v = np.asarray(v, F32).astype(np.float64)
    o1, o2 = float(F32(omb1)), float(F32(omb2))
    ms = m + (g - m) * o1
    vs = v + (g * g - v) * o2
    delta = ms * float(F32(alpha)) / (np.sqrt(vs) + float(F32(eps)))
    return p - delta, ms, vs, delta


def replay(p, m, v, alphas, omb1, omb2, eps=1e-8, two_l2=0.0):
    """L steps, one per alpha, gradient 0 (or the regulariser's two_l2 p alone), along the EXACT trajectory (float64, no
    rounding between the steps): (p, m, v) after the last step and the bars of a site that rounds every step with the
    hardware recipe -- each step's own bar plus the earlier steps' slot errors, decayed by beta and carried into the
    step's delta (p in float64)."""
    p, m, v = (np.asarray(x, F32).astype(np.float64) for x in (p, m, v))
    bp, bm, bv = (np.zeros(p.shape) for _ in range(3))
    o1, o2 = float(F32(omb1)), float(F32(omb2))
    b1, b2 = 1.0 - o1, 1.0 - o2
    for a in alphas:
        g = two_l2 * p
        ms = m + (g - m) * o1
        vs = v + (g * g - v) * o2
        den = np.sqrt(vs) + float(F32(eps))
        d = ms * float(F32(a)) / den
        # this step's roundings; the error already in m / v decays with the slot (x beta); an error in p moves the
        # regulariser's gradient by two_l2 |p error|
        bm = b1 * bm + slot_bar(ms, (g - m) * o1, k=2) + o1 * (U * np.abs(g) + two_l2 * bp)    # (+ fl(two_l2 p))
        bv = b2 * bv + slot_bar(vs, (g * g + np.abs(v)) * o2, k=3)
        with np.errstate(divide="ignore", invalid="ignore"):
            carry = float(F32(a)) * bm / den + np.where(vs > 0, np.abs(d) * bv / (2 * np.where(vs > 0, vs, 1)), 0.0)
        bp = bp + half_ulp(p - d) + K_HW * U * np.abs(d) + carry
        p, m, v = p - d, ms, vs
    return p, m, v, (bp, bm, bv)


def ulp(x):
    """fp32 ulp at |x| (float64 in, float64 out); the denormal spacing below 2^-126."""
    a = np.abs(np.asarray(x, np.float64)).astype(F32)
    return np.spacing(a).astype(np.float64)


def half_ulp(x):
    """half an fp32 ulp at the larger of the two floats around x."""
    a = np.abs(np.asarray(x, np.float64))
    lo = a.astype(F32)
    hi = np.nextafter(lo, F32(np.inf))
    return 0.5 * np.maximum(np.spacing(lo), np.spacing(hi)).astype(np.float64)


def slot_bar(exact, incr, k=2):
    """0.5 ulp(x*) + k u |increment| (see the module docstring)."""
    return half_ulp(exact) + k * U * np.abs(incr)


def bars(g, p, m, v, alpha, omb1, omb2, eps=1e-8, two_l2=0.0, hw=False, m_got=None, v_got=None):
    """exact (p*, m*, v*) and the three bars of one step.  m_got / v_got: the site's own slots (their error is carried
    into the parameter's bar); None = the exact ones."""
    ps, ms, vs, d = step(g, p, m, v, alpha, omb1, omb2, eps, two_l2)
    gk = np.asarray(g, F32)
    if two_l2:
        gk = ((F32(two_l2) * np.asarray(p, F32)).astype(F32) + gk).astype(F32)
    gk = gk.astype(np.float64)
    m64 = np.asarray(m, F32).astype(np.float64)
    v64 = np.asarray(v, F32).astype(np.float64)
    bm = slot_bar(ms, (gk - m64) * float(F32(omb1)), k=2)
    bv = slot_bar(vs, (gk * gk + np.abs(v64)) * float(F32(omb2)), k=3)
    em = 0.0 if m_got is None else np.abs(np.asarray(m_got, F32).astype(np.float64) - ms)
    ev = 0.0 if v_got is None else np.abs(np.asarray(v_got, F32).astype(np.float64) - vs)
    den = np.sqrt(vs) + float(F32(eps))
    with np.errstate(divide="ignore", invalid="ignore"):
        carry = float(F32(alpha)) * em / den + np.where(vs > 0, np.abs(d) * ev / (2 * np.where(vs > 0, vs, 1)), 0.0)
    bp = half_ulp(ps) + (K_HW if hw else K_IEEE) * U * np.abs(d) + carry
    return (ps, ms, vs), (bp, bm, bv)


def excess(got, exact, bar):
    """|got - exact| / bar, elementwise (<= 1 passes).  A result that is denormal in fp32 may also be 0."""
    got = np.asarray(got, F32).astype(np.float64)
    exact = np.asarray(exact, np.float64)
    err = np.abs(got - exact)
    ftz = (np.abs(exact) < TINY) & (got == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    return np.where(ftz, 0.0, r)


def ulps(got, exact):
    """|got - exact| in ulps of the exact value."""
    got = np.asarray(got, F32).astype(np.float64)
    exact = np.asarray(exact, np.float64)
    return np.abs(got - exact) / np.maximum(ulp(exact), 2.0 ** -149)
