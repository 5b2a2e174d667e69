"""Saturated predictions for the loss heads (test infrastructure; not a test).

The Keras BCE clips p to [1e-7, 1 - 1e-7] and the clip's zero gradient multiplies d loss / d logit
(`inside`).  At the suite's initial values |logit| < 1 and every row is inside the clip.  This module makes a tower
saturate and picks the rows of a batch by class, from the ORACLE's logits alone:

    class            range                  what it is
    normal           |z| <= 6               inside the clip, well conditioned
    saturated high   20 <= z <= 80          p rounds to 1.0f, exp(-z) still a normal number
    saturated low    -80 <= z <= -20        p = exp(z) < 1e-7
    extreme          100 <= |z| <= 1000     exp underflows: p is exactly 1 on the high side, 0 or a denormal on the low one

No row of a batch may lie in 6 < |z| < 20.  Above |z| = 6 one ulp of p moves the loss of a far-side label by
2^-24 (1 + e^|z|) (1.8e-4 at 8, 9.6e-3 at 12), and between 15 and 17.5 the fp32 p walks the grid 1 - k 2^-24 across the
clip boundary 1 - 2^-23: such a row tests the rounding of `__expf` and of one division, in the oracle and in the kernel
alike, not the head.  This is a condition on the reference, asserted here, never measured on the device.

1. `saturate` scales the output unit (`wo`, or `head_<d>/w` of a multi-task kind), element by element, and sets the global
   bias so that the oracle's logits over one domain spread from below -100 to above +100 (why not by one factor: see
   there).  The caller packs the oracle's parameters into the engine afterwards: both sides hold the same scaled tensors.
2. `pick` chooses the rows of one batch for `train_steps(perm=...)`, `pick_eval` those of an evaluation split.  Dropout
   masks depend on the batch position and PartitionedNorm's statistics on the whole batch, so the oracle's logits are
   computed for the candidates where they would sit, and recomputed for the chosen order; an offending row is replaced by
   the next candidate, in bounded deterministic loops; the conditions are asserted at the end (`assert_conditions`).

`Problem` is what both need from one of the suite's oracles (oracle/tower.py, fmnets.py, mtl.py, star.py,
tests/star_forms_ref.py): every one of them ends its forward in `oracle.tower.sigmoid(logit)`, which is where the logits
are read (`logits_seen`); the oracles themselves stay untouched.
"""
import contextlib

import numpy as np

from oracle import tower as otower

F32 = np.float32
NORMAL_MAX = 6.0
SAT_MIN, SAT_MAX = 20.0, 80.0
EXT_MIN, EXT_MAX = 100.0, 1000.0

# the oracle's per-row loss of a clipped row (oracle.tower.bce_per_row; a constant: only __logf's error remains on the device)
LOSS_HIGH_Y0, LOSS_HIGH_Y1 = 15.9424, 1.19e-7
LOSS_LOW_Y1, LOSS_LOW_Y0 = 16.1181, 1.0e-7

# A layout lists one slot per batch row; a slot is a tuple of acceptable (class, label) pairs, label None = any.  N normal,
# H / L saturated high / low, XH / XL extreme high / low.
def _one(c, y=None):
    return ((c, y),)


# 24 rows = one and a half 16-row tiles, six 4-row tiles: 8 normal rows, every saturated and extreme class with either
# label (16 rows).  Without dropout slot i is batch row i: every 4-row tile and both 16-row tiles are mixed and the last row
# before the padding is saturated the wrong way.  With dropout the mask of a batch row shifts every candidate's logit at
# that row by the same large amount, some classes cannot occur there, and `pick` deals the slots to the rows that can hold
# them (`free`).
MIXED = [_one("N"), _one("H", 0), _one("L", 1), _one("XH", 0), _one("N"), _one("XL", 1), _one("H", 1), _one("L", 0),
         _one("N"), _one("XH", 1), _one("L", 1), _one("N"), _one("H", 0), _one("N"), _one("L", 0), _one("H", 1),
         _one("N"), _one("L", 1), _one("H", 1), _one("N"), _one("L", 0), _one("N"), _one("XL", 0), _one("H", 0)]
# the wrong way: label 0 with p -> 1 (the largest p - y there is), label 1 with p -> 0
WRONG_WAY = (("H", 0), ("XH", 0), ("L", 1), ("XL", 1))
CLIPPED = WRONG_WAY + (("H", 1), ("XH", 1), ("L", 0), ("XL", 0))
# one 4-row tile plus one row, every row clipped; the first, the second and the remainder row the wrong way
ALL_SATURATED_5 = [WRONG_WAY, WRONG_WAY, CLIPPED, CLIPPED, WRONG_WAY]
# the remainder row alone, the wrong way
ALL_SATURATED_1 = [WRONG_WAY]


def classify(z):
    """class name per logit; "" for a logit in no class (6 < |z| < 20, 80 < |z| < 100, |z| > 1000, not finite)."""
    z = np.asarray(z, np.float64)
    out = np.full(z.shape, "", dtype=object)
    a = np.abs(z)
    out[a <= NORMAL_MAX] = "N"
    out[(z >= SAT_MIN) & (z <= SAT_MAX)] = "H"
    out[(z <= -SAT_MIN) & (z >= -SAT_MAX)] = "L"
    out[(z >= EXT_MIN) & (z <= EXT_MAX)] = "XH"
    out[(z <= -EXT_MIN) & (z >= -EXT_MAX)] = "XL"
    return out


def fits(slot, cls, label):
    return any(cls == c and (y is None or int(label) == y) for c, y in slot)


def assert_conditions(z, cls, labels, layout, free=False):
    """the issue's conditions on one batch, on the oracle's logits `z` and their classes `cls` (Problem.train_classes /
    eval_classes) in batch order.  free: the slots may sit at any row."""
    z, labels = np.asarray(z, np.float64), np.asarray(labels)
    a = np.abs(z)
    assert z.shape[0] == len(layout) and np.isfinite(z).all()
    assert not np.any((a > NORMAL_MAX) & (a < SAT_MIN)), z          # the ill-conditioned band holds no row
    assert np.all(cls != ""), (z, cls)
    assert np.array_equal(cls == "N", a <= NORMAL_MAX)
    if free:            # the rows hold the layout's slots in some order: every slot is one (class, label) pair here
        have = sorted((c, -1 if c == "N" else int(y)) for c, y in zip(cls, labels))
        assert have == sorted((c, -1 if y is None else y) for (c, y), in layout), have
    else:
        for i, slot in enumerate(layout):
            assert fits(slot, cls[i], labels[i]), (i, slot, float(z[i]), labels[i])
    if len(layout) == len(MIXED):
        for c in ("H", "L", "XH", "XL"):
            for y in (0, 1):
                assert np.any((cls == c) & (labels == y)), (c, y)
        assert int(np.sum(cls == "N")) == 8


@contextlib.contextmanager
def logits_seen():
    """the logits of every oracle forward run inside the block (a list of fp32 arrays, one per call)."""
    seen, real = [], otower.sigmoid

    def spy(z):
        seen.append(np.array(z, F32))
        return real(z)
    otower.sigmoid = spy
    try:
        yield seen
    finally:
        otower.sigmoid = real


class Problem(object):
    """one oracle model, one domain's train split, and the calls that differ between the oracles.

    family: "tower" (oracle/tower.py), "fm" (oracle/fmnets.py), "mtl" (oracle/mtl.py), "star" (oracle/star.py),
    "starform" (tests/star_forms_ref.StarForms)."""

    def __init__(self, family, model, cols, domain, spec=None):
        self.family, self.model, self.cols, self.d, self.spec = family, model, cols, int(domain), spec
        mt = family == "mtl"
        self.w_name, self.gb_name = ("head_%d/w" % self.d, "head_%d/gb" % self.d) if mt else ("wo", "gb")
        self.rate = 0.0 if family in ("star", "starform") else float(model.rate)
        self.big = ()           # the units of the output kernel that `saturate` gave large weights

    @property
    def params(self):
        return self.model.params

    def batch(self, idx):
        c = self.cols
        return c["uid"][idx], c["pid"][idx], c["domain"][idx], c["label"][idx]

    def loss_and_grads(self, idx, step):
        """-> (loss, grads, logits) of the training batch cols[idx] at dropout step `step`; nothing is updated."""
        m, (uid, pid, dom, label) = self.model, self.batch(np.asarray(idx))
        B = len(idx)
        with logits_seen() as seen:
            if self.family == "tower":
                masks = otower.train_masks(m.seed, step, B, m.hidden, m.rate) if m.rate > 0 else \
                    [np.ones((B, h), F32) for h in m.hidden]
                loss, g = otower.loss_and_grads(m.params, uid, pid, dom, label, masks, m.rate, m.emb_trainable,
                                                m.frozen_sumsq(), m.deepfm, m.uncertainty, m.l2)[:2]
            elif self.family == "fm":
                from oracle import fmnets as ofm
                masks = otower.train_masks(m.seed, step, B, m.hidden, m.rate) if m.rate > 0 else None
                fn = ofm.loss_and_grads_conv if m.conv else ofm.loss_and_grads
                loss, g = fn(m.params, m.kind, uid, pid, dom, label, masks, m.rate, m.emb_trainable, m.frozen_sumsq(),
                             m.uncertainty, m.l2)[:2]
            elif self.family == "mtl":
                from oracle import mtl as omtl
                masks = omtl.train_masks(self.spec, m.seed, step, B, m.rate) if m.rate > 0 else None
                loss, g = omtl.loss_and_grads(m.params, self.spec, self.d, uid, pid, dom, label, masks, m.rate,
                                              m.emb_trainable, m.frozen_sumsq(), m.l2)[:2]
            elif self.family == "star":
                from oracle import star as ostar
                loss, g = ostar.loss_and_grads(m.params, m.state, uid, pid, dom, label, m.emb_trainable)[:2]
            elif self.family == "starform":
                loss, g = m.loss_and_grads(uid, pid, dom, label)[:2]
            else:
                raise ValueError(self.family)
        assert len(seen) == 1 and seen[0].shape == (B,)
        return loss, g, seen[0]

    def train_logits(self, idx, step):
        """the logits of loss_and_grads(idx, step) (the same forward, without the backward pass where the oracle has one
        apart)."""
        from oracle import rng as orng
        m, (uid, pid, dom, label) = self.model, self.batch(np.asarray(idx))
        B = len(idx)
        keep = orng.keep_scale(m.rate) if self.rate > 0 else F32(1)
        with logits_seen() as seen:
            if self.family == "star":
                from oracle import star as ostar
                ostar.forward(m.params, m.state, uid, pid, dom, True)
            elif self.family == "starform":
                import star_forms_ref as sref
                sref.forward(m.params, m.state, uid, pid, dom, True, m.norm, m.dense, m.auxiliary_dim)
            elif self.family == "tower":
                masks = otower.train_masks(m.seed, step, B, m.hidden, m.rate) if m.rate > 0 else None
                otower.forward(m.params, uid, pid, dom, masks, keep, m.deepfm)
            elif self.family == "fm":
                from oracle import fmnets as ofm
                masks = otower.train_masks(m.seed, step, B, m.hidden, m.rate) if m.rate > 0 else None
                (ofm.forward_conv if m.conv else ofm.forward)(m.params, m.kind, uid, pid, dom, masks, keep)
            else:
                from oracle import mtl as omtl
                masks = omtl.train_masks(self.spec, m.seed, step, B, m.rate) if m.rate > 0 else None
                omtl.forward(m.params, self.spec, self.d, uid, pid, dom, masks, keep)
        assert len(seen) == 1 and seen[0].shape == (B,)
        return seen[0]

    def evaluate(self, cols, batch):
        """the oracle's evaluation of a split -> (loss, predictions, logits)."""
        with logits_seen() as seen:
            loss, preds = self.model.evaluate(self.d, cols, batch) if self.family == "mtl" else self.model.evaluate(cols, batch)
        return loss, preds, np.concatenate(seen)

    @contextlib.contextmanager
    def big_units_off(self):
        """the output unit without the large weights `saturate` gave it."""
        w = self.params[self.w_name]
        keep = w[list(self.big)].copy()
        w[list(self.big)] = 0
        try:
            yield
        finally:
            w[list(self.big)] = keep

    def train_classes(self, idx, step):
        """-> (training logits, their classes); a row counts as normal only if its logit is the same BITS without the large
        weights: the units that carry them are exactly zero there, not cancelling each other."""
        z = self.train_logits(idx, step)
        with self.big_units_off():
            body = self.train_logits(idx, step)
        cls = classify(z)
        cls[(cls == "N") & (z != body)] = ""
        return z, cls

    def eval_classes(self, cols, batch):
        z = self.evaluate(cols, batch)[2]
        with self.big_units_off():
            body = self.evaluate(cols, batch)[2]
        cls = classify(z)
        cls[(cls == "N") & (z != body)] = ""
        return z, cls


def saturate(prob, step=0, inference=False, body=3.0, sat=45.0, ext=220.0):
    """scale the output unit, element by element, and set the global bias so that the oracle's logits over the domain's
    train split hold every class and reach below -100 and above +100 (asserted) -> (those logits, their classes).  The
    logits are the training ones of the split as one batch at dropout step `step`, or (`inference`) the evaluation's.

    ONE factor for the whole kernel would do that too, and was tried first: a spread of 50 needs a factor of 100 .. 500,
    a normal row is then a sum of 64 terms of size ~10 that cancel to |z| <= 6, and the factor multiplies the fp32 rounding
    of the last hidden layer as well -- the oracle's own logits of such rows differ from a float64 forward by up to 6e-5
    (measured; the prediction bar is rtol 2e-5).  Every normal row would test rounding, which is what the band
    6 < |z| < 20 is left out for.  So the kernel is scaled by one moderate factor (the part of the logit it carries gets
    standard deviation `body`: normal rows spread over a few units instead of |z| < 1), and FOUR of its units -- the ones
    that relu leaves on least often, but on at least 8 % of the rows -- get large weights instead:
    +sat / -sat and +ext / -ext over the median of their non-zero activations.  A row with all four units off is a normal
    row as well conditioned as any row of the suite (the large weights multiply exact zeros); a row with one on is saturated
    or extreme, whatever the rounding.  The bias centres the rows with all four off at zero."""
    P = prob.params
    n = prob.cols["uid"].shape[0]
    idx = np.arange(n)

    def logits():
        z = prob.evaluate(prob.cols, n)[2] if inference else prob.train_logits(idx, step)
        return z.astype(np.float64)
    w, gb = P[prob.w_name], P[prob.gb_name]
    w0 = w.copy()
    gb[...] = 0
    w[...] = 0
    rest = logits()                                 # what the output unit does not carry (FM, linear part)
    w[...] = w0
    carried = logits() - rest
    assert carried.std() > 0
    w_new = (w0.astype(np.float64) * min(body / carried.std(), 32.0))
    # how often relu leaves each unit on, from the inference logits of the split's first rows (a unit that only dropout
    # switches off is on or off for EVERY candidate of a batch row: no use)
    head = {k: v[:400] for k, v in prob.cols.items()}

    def probe():            # (without dropout the logits of the mode itself: a norm layer's statistics differ between the two)
        return prob.evaluate(head, 400)[2].astype(np.float64) if prob.rate > 0 else logits()
    w[...] = 0
    rest_inf = probe()
    frac = np.zeros(w0.shape[0])
    for j in range(w0.shape[0]):
        w[...] = 0
        w[j] = 1
        frac[j] = np.mean(probe() != rest_inf)
    big = [int(j) for j in np.argsort(frac, kind="stable") if frac[j] >= 0.08][:4]
    assert len(big) == 4 and frac[big[-1]] <= 0.65, (big, frac[big])
    act = np.zeros((n, 4))
    for k, (j, weight) in enumerate(zip(big, (sat, -sat, ext, -ext))):
        w[...] = 0
        w[j] = 1
        t = logits() - rest                         # unit j's activation of every row (exact zeros kept)
        assert np.all(t >= 0) and np.any(t > 0), j
        w_new[j] = weight / np.median(t[t > 0])
        act[:, k] = t
    w[...] = w_new.astype(F32)
    off = ~np.any(act != 0, axis=1)
    assert off.sum() >= 16, int(off.sum())
    gb[...] = F32(-np.median(logits()[off]))
    prob.big = tuple(big)
    z, cls = prob.eval_classes(prob.cols, n) if inference else prob.train_classes(idx, step)
    assert z.min() < -EXT_MIN and z.max() > EXT_MIN, (float(z.min()), float(z.max()))
    return z, cls


def _pick_by_row(prob, layout, step, used, candidates):
    """dropout on: the logit of a candidate depends on the batch row it sits at.  The first `candidates` rows of the split
    are evaluated at every batch row (one forward per candidate, the batch rolled); a layout of single-pair slots is dealt
    to the batch rows by a matching (`free`), row i of any other layout keeps slot i.  -> idx, or None where this step's
    masks leave some slot without a batch row or a candidate."""
    labels = np.asarray(prob.cols["label"])
    n, B = labels.shape[0], len(layout)
    free = all(len(slot) == 1 for slot in layout)
    C = min(n, max(int(candidates), B))
    cls = np.full((C, B), "", dtype=object)
    for k in range(C):
        rows = (k + np.arange(B)) % C
        cls[rows, np.arange(B)] = prob.train_classes(rows, step)[1]
    lab = labels[:C, None]
    # ok[s][r, i]: candidate r at batch row i fits slot s
    ok = [np.any([(cls == c) & (True if y is None else lab == y) for c, y in slot], axis=0) for slot in layout]
    avail = np.array([r not in used for r in range(C)])

    def fit(s, i):
        return np.nonzero(ok[s][:, i] & avail)[0]
    row_of = list(range(B))                         # slot -> batch row
    if free:                                        # a matching of slots and batch rows (augmenting paths, fixed order)
        edge = np.array([[fit(s, i).size >= 2 for i in range(B)] for s in range(B)])
        slot_at = [-1] * B

        def place(s, seen):
            for i in range(B):
                if edge[s, i] and i not in seen:
                    seen.add(i)
                    if slot_at[i] < 0 or place(slot_at[i], seen):
                        slot_at[i] = s
                        return True
            return False
        for s in sorted(range(B), key=lambda s: (int(edge[s].sum()), s)):
            if not place(s, set()):
                return None
        for i, s in enumerate(slot_at):
            row_of[s] = i
    idx = np.full(B, -1, np.int64)
    for s in range(B):
        cand = fit(s, row_of[s])
        if not cand.size:
            return None
        idx[row_of[s]] = cand[0]
        avail[cand[0]] = False
    return idx


def _pick_in_order(prob, layout, step, used, guess, max_rounds=400):
    """dropout off: batch row i holds slot i.  Rows that fitted a slot in `guess` (classes of all rows from an earlier
    forward) are tried first, the logits are recomputed for the chosen batch, and while some row does not fit its slot the
    first candidate that makes more rows of the batch fit takes the place of the first such row (a norm layer's batch
    statistics couple the rows: a replacement moves every logit of the batch; elsewhere the first candidate of the right
    class is accepted at once)."""
    labels = np.asarray(prob.cols["label"])
    n, B = labels.shape[0], len(layout)
    queues = []
    for slot in layout:
        ok = np.array([fits(slot, guess[r], labels[r]) for r in range(n)])
        lab = np.array([any(y is None or int(labels[r]) == y for _, y in slot) for r in range(n)])
        queues.append([int(r) for r in np.nonzero(ok)[0]] + [int(r) for r in np.nonzero(lab & ~ok)[0]])

    def fitting(idx):
        cls = prob.train_classes(idx, step)[1]
        return [fits(layout[i], cls[i], labels[idx[i]]) for i in range(B)]
    idx = np.zeros(B, np.int64)
    for i in range(B):
        idx[i] = next(r for r in queues[i] if r not in used)
        used.add(int(idx[i]))
    good = fitting(idx)
    for rounds in range(max_rounds):
        if all(good):
            return idx
        for i in [i for i in range(B) if not good[i]]:
            for r in queues[i][:300]:
                if r in used:
                    continue
                trial = idx.copy()
                trial[i] = r
                g2 = fitting(trial)
                if g2[i] and sum(g2) >= sum(good) + (rounds % 2):     # (every other round a sideways move will do)
                    used.discard(int(idx[i]))
                    used.add(r)
                    idx, good = trial, g2
                    break
            else:
                continue
            break
        else:
            if rounds % 2 == 0:                     # not even a sideways move is left
                return None
    return None


def pick(prob, layout, step, guess=None, exclude=(), candidates=400, steps=8):
    """rows of the domain's train split for one batch that holds `layout` under the oracle's TRAINING logits ->
    (dropout step, idx int32 [len(layout)], logits).  Deterministic: candidates are taken in file order.  With dropout the
    masks of a step can leave a slot without any batch row that can hold it (all four large units dropped at a row: every
    candidate is normal there); the next dropout step is tried then, `steps` of them from `step` on, and the caller sets
    the engine's dropout counter to the step returned."""
    labels = np.asarray(prob.cols["label"])
    for st in range(step, step + (steps if prob.rate > 0 else 1)):
        used = set(int(e) for e in exclude)         # rows of this batch (and the caller's): a row is taken once
        if prob.family in ("star", "starform") and len(layout) == 1:
            # a norm layer's batch statistics map a batch of ONE row to its offset beta: the logit is the same number for
            # every row of the split.  The global bias is MOVED here so that it is +45 (the caller packs the parameters
            # again), and the first unused row with label 0 is the wrong-way row
            assert (("H", 0),) == layout[0][:1]
            idx = np.array([next(r for r in range(labels.shape[0]) if r not in used and labels[r] == 0)], np.int64)
            prob.params[prob.gb_name][...] += F32(45.0) - prob.train_logits(idx, st)[0]
        elif prob.rate > 0:
            idx = _pick_by_row(prob, layout, st, used, candidates)
        else:
            idx = _pick_in_order(prob, layout, st, used, guess if guess is not None else np.full(labels.shape[0], "", dtype=object))
        if idx is not None:
            break
    assert idx is not None, ("no batch for", layout)
    z, cls = prob.train_classes(idx, st)
    assert np.array_equal(z, prob.loss_and_grads(idx, st)[2])       # the very call the tests take their reference from
    assert_conditions(z, cls, labels[idx], layout, prob.rate > 0 and all(len(slot) == 1 for slot in layout))
    return st, idx.astype(np.int32), z


def pick_eval(prob, cols, layout, batch=256):
    """rows of an evaluation split, by the oracle's inference logits (no dropout; a norm layer's moving statistics: nothing
    depends on the position) -> (idx [len(layout)] in layout order, their logits)."""
    z, cls = prob.eval_classes(cols, batch)
    labels = np.asarray(cols["label"])
    idx = []
    for slot in layout:
        cand = [r for r in range(z.shape[0]) if r not in idx and fits(slot, cls[r], labels[r])]
        assert cand, ("no row for", slot)
        idx.append(cand[0])
    idx = np.array(idx, np.int64)
    assert_conditions(z[idx], cls[idx], labels[idx], layout)
    return idx, z[idx]


def loss_slack(z, normal, ulps):
    """the part of a batch-mean loss bar that `ulps` ulps of p on the normal rows are worth: one ulp of p moves the loss of a
    row by at most 2^-24 (1 + e^|z|) (d loss / d p = 1 / (1 - p) or 1 / p; p's ulp is at most 2^-24 below 1)."""
    z = np.asarray(z, np.float64)
    return ulps / float(z.shape[0]) * float(np.sum(2.0 ** -24 * (1.0 + np.exp(np.abs(z[normal])))))


def ulp_distance(a, b):
    """|a - b| in units in the last place of fp32, elementwise (finite values of one sign, as predictions are)."""
    ia = np.asarray(a, F32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, F32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
