"""Generate tests/golden/pcgrad_shape_goldens.npz from the reference's OWN numpy method
`PCGrad.PCGrad(final_grads, current_grads, aux_grads)` (model_zoo/pcgrad.py:152-160) at every family of variable
shapes the engines produce -- a second file beside pcgrad_goldens.npz with its own seed, so that file's random
stream (and its committed arrays) stay as they are.

Built like make_pcgrad_goldens.py: the reference's class is imported at run time behind the stub finder of
make_outer_goldens.py, `final_grads` IS `current_grads` (pcgrad.py:101-102), and two auxiliary gradients are
projected one after the other.  Only arrays go into the .npz.

Shapes: every regime of numpy's pairwise summation along the last axis (n < 8; 8 <= n <= 128 with and without a
tail; the recursion above 128 with its `n2 -= n2 % 8`; 4096, the kernel's cap), 1-d variables (the reference's
mask is 0-d there), 3-d variables (Star's [D, in, out]) and a [n, 1] variable.  SPECIAL tensors carry rows with
chosen data (see `special_rows`); `main` asserts of the denormal rows that they are what their names say.

Size: about 0.9 MB, five times pcgrad_goldens.npz, and deliberately so.  Seven arrays of random fp32 per tensor
do not compress; the 1000- and 4096-wide tensors are already cut from 5 rows to 2 (the second row is what shows
a kernel that strides rows wrongly at the longest slice), and every other tensor is one case of the list above.

Usage:  python tests/golden/make_pcgrad_shape_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_outer_goldens as mog  # noqa: E402  (stub finder)

OUT = os.path.join(HERE, "pcgrad_shape_goldens.npz")
WIDTHS = (2, 3, 4, 7, 8, 9, 15, 16, 17, 32, 96, 127, 129, 136, 160, 192, 255, 257, 320, 384, 512)
SHAPES = ([(5, n) for n in WIDTHS] + [(2, 1000), (2, 4096)]
          + [(n,) for n in (4, 7, 8, 9, 384, 512)]
          + [(3, 5, 64), (2, 7, 32), (300, 1)]
          # the tensors with special rows: 2-d (eight rows: one per kind), 3-d (the first eight slices), 1-d (one kind each)
          + [(8, 128), (8, 384), (3, 5, 64)] + [(128,)] * 8)
N_PLAIN = len(WIDTHS) + 2 + 6 + 3
KINDS = ("cur_zero", "aux_zero", "dot_neg", "dot_pos", "equal", "scale_1e-20", "denormal_dot", "denormal_norm")
TINY = np.finfo(np.float32).tiny                 # 1.1754944e-38: what lies below is denormal


def special_rows(kind, cur, a1, a2):
    """one slice (1-d views of the three gradients) of the given kind, in place:
    cur_zero  the running gradient is all zero (dot 0: not projected; the sum is the auxiliary gradient)
    aux_zero  both auxiliary gradients are all zero
    dot_neg   dot < 0 for the first auxiliary gradient (every product negative)
    dot_pos   dot > 0 (every product positive)
    equal     the first auxiliary gradient IS the running gradient
    scale_1e-20    all three at scale 1e-20 with dot > 0: every product is an fp32 denormal (the squared norm too up to
                   about 100 columns).  The reference subtracts dot / ||cur|| * cur, about sqrt(n) * 1e-40 here, far below
                   one ulp of an auxiliary gradient at 1e-20: this row pins only that NOTHING moves, and a kernel that
                   flushes denormals passes it.  The next two rows are the ones that tell.
    denormal_dot   cur at 1e-5, the auxiliary gradients at 1e-36, every product of the first positive: the products and
                   the dot product are denormal, the squared norm is normal, and what is subtracted is about 1e-4 of the
                   auxiliary gradient -- products flushed to zero give dot 0 and no projection, other bytes
    denormal_norm  cur at 1e-21, so the squared norm is denormal as well; the auxiliary gradient at 1e-36 but for three
                   elements at 1e-18, whose products (denormal) make the dot product (denormal); what is subtracted
                   (denormal) is again about 1e-4 of the small elements -- a squared norm flushed to zero divides by 0"""
    if kind == "cur_zero":
        cur[...] = 0
    elif kind == "aux_zero":
        a1[...] = 0
        a2[...] = 0
    elif kind == "dot_neg":
        a1[...] = -np.abs(a1) * np.sign(cur)
    elif kind == "dot_pos":
        a1[...] = np.abs(a1) * np.sign(cur)
    elif kind == "equal":
        a1[...] = cur
    elif kind == "scale_1e-20":
        cur *= np.float32(1e-18)          # (the values are N(0, 1) * 0.01)
        a1[...] = np.abs(a1) * np.sign(cur) * np.float32(1e-18)
        a2 *= np.float32(1e-18)
    elif kind == "denormal_dot":
        cur *= np.float32(1e-3)
        a1[...] = np.abs(a1) * np.sign(cur) * np.float32(1e-34)
        a2 *= np.float32(1e-34)
    elif kind == "denormal_norm":
        big = [1, cur.size // 3, cur.size - 2]
        cur *= np.float32(1e-19)
        for a in (a1, a2):
            large = a[big] * np.float32(1e-16)
            a *= np.float32(1e-34)
            a[big] = large
        a1[...] = np.abs(a1) * np.sign(cur)
    else:
        raise ValueError(kind)


def check_denormal_row(kind, cur, a1, a1_after):
    """the two rows that tell are what they claim: denormal products / dot product / squared norm, and a projection
    that changes the auxiliary gradient -- else a kernel that flushes or skips them would leave the same bytes"""
    prod, dot, nrm2 = cur * a1, np.sum(cur * a1), np.sum(cur * cur)
    assert 0 < np.abs(prod).max() < TINY and 0 < dot < TINY, (kind, np.abs(prod).max(), dot)
    assert (0 < nrm2 < TINY) if kind == "denormal_norm" else nrm2 > TINY, (kind, nrm2)
    moved = a1_after.view(np.uint32) != a1.view(np.uint32)
    assert moved.mean() > 0.9, (kind, moved.mean())
    return moved.mean()


def main():
    sys.meta_path.insert(0, mog._StubFinder())
    sys.path.insert(0, mog.REF)
    from model_zoo.pcgrad import PCGrad
    obj = PCGrad.__new__(PCGrad)
    rs = np.random.RandomState(20240917)

    def rand():
        return [(rs.standard_normal(s) * 0.01).astype(np.float32) for s in SHAPES]

    current, aux1, aux2 = rand(), rand(), rand()
    kinds = np.full(len(SHAPES), -1, np.int32)         # per tensor: -1 plain, -2 every kind in its first slices, else the kind
    one_d = 0
    for i in range(N_PLAIN, len(SHAPES)):
        c, a1, a2 = current[i], aux1[i], aux2[i]
        if c.ndim == 1:
            kinds[i] = one_d % len(KINDS)
            special_rows(KINDS[kinds[i]], c, a1, a2)
            one_d += 1
        else:
            kinds[i] = -2
            n = c.shape[-1]
            for r, kind in enumerate(KINDS):
                special_rows(kind, c.reshape(-1, n)[r], a1.reshape(-1, n)[r], a2.reshape(-1, n)[r])
    out = {"n_tensors": np.array(len(SHAPES)), "kinds": kinds}
    for i, (c, a1, a2) in enumerate(zip(current, aux1, aux2)):
        out["current_%d" % i], out["aux1_%d" % i], out["aux2_%d" % i] = c.copy(), a1.copy(), a2.copy()
    final = current                                 # the same list object, as in pcgrad.py:101-102
    with np.errstate(all="ignore"):
        obj.PCGrad(final, current, aux1)
        for i in range(len(SHAPES)):
            out["after1_final_%d" % i], out["after1_aux_%d" % i] = final[i].copy(), aux1[i].copy()
        obj.PCGrad(final, current, aux2)
        for i in range(len(SHAPES)):
            out["after2_final_%d" % i], out["after2_aux_%d" % i] = final[i].copy(), aux2[i].copy()
    with np.errstate(all="ignore"):
        for i in np.nonzero(kinds != -1)[0]:
            n = SHAPES[i][-1]
            for r, kind in enumerate(KINDS) if kinds[i] == -2 else [(0, KINDS[kinds[i]])]:
                if kind.startswith("denormal"):
                    check_denormal_row(kind, *[out["%s_%d" % (k, i)].reshape(-1, n)[r] for k in ("current", "aux1", "after1_aux")])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(out), "arrays", len(SHAPES), "tensors", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
