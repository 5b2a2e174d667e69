"""What k_wgrad_adam hands to the next tower: the S workgroups read their pre-update block of W0[256:384] from the live
parameters (no snapshot), W1^T is only kept where a tower can read it, and every stepped element is stored exactly once.

The engines are built on small problems of this file's own (engine.TowerEngine directly): the domain count decides how
many 16-row one-hot blocks the S workgroups contract (1, 10, 17, 33 domains = one, one, two, three blocks).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import tower as otower      # noqa: E402

F32 = np.float32
N_USER = N_ITEM = 64


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine
    return engine


def make_inputs(n_domain, passes, seed):
    """parameters, frozen tables and the train splits {domain id: columns}; passes: {domain id: (rows, domain column:
    None = the domain id itself, "mixed" = every domain id in turn, shuffled)}.  Both labels occur in every split of two
    rows or more."""
    rs = np.random.RandomState(seed)
    params = otower.init_params(rs, N_USER, N_ITEM, n_domain)
    params["domain_emb"] = (rs.standard_normal(params["domain_emb"].shape) * 0.05).astype(F32)
    for l in range(3):
        params["b%d" % l] = (rs.standard_normal(params["b%d" % l].shape) * 0.05).astype(F32)
    data = {}
    for d, (rows, col) in passes.items():
        dom = np.full(rows, d, np.int32) if col is None else rs.permutation(np.arange(rows) % n_domain).astype(np.int32)
        label = rs.permutation(np.arange(rows) % 2).astype(F32)
        data[d] = {"uid": rs.randint(0, N_USER, rows).astype(np.int32), "pid": rs.randint(0, N_ITEM, rows).astype(np.int32),
                   "domain": dom, "label": label}
    return params, data


def make_engine(engine, n_domain, batch, params, data, dropout=0.5, switches=None, tower_tile=None):
    """(the library reads its switches when the context is created)"""
    switches = switches or {}
    os.environ.update(switches)
    try:
        eng = engine.TowerEngine(N_USER, N_ITEM, n_domain, batch, dropout=dropout, tower_tile=tower_tile)
    finally:
        for k in switches:
            os.environ.pop(k, None)
    eng.bind_table("user_emb", params["user_emb"])
    eng.bind_table("item_emb", params["item_emb"])
    for d, c in data.items():
        eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
    eng.set_weights(eng.pack(params))
    return eng


def host(t):
    return t.cpu().numpy().copy()


def state(eng):
    return host(eng.get_weights()), host(eng.adam_m), host(eng.adam_v)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def assert_adam_close(got, want, n_steps, lr, name, max_frac=2e-3):
    """the multi-step Adam bar of tests/test_gpu_parity.py (see there), as test_fused_wgrad_adam_matches_the_slab_path
    applies it: all but max_frac of the elements within 5 % of k lr, none beyond 2 k lr, the median far tighter."""
    diff = np.abs(np.asarray(got, F32).ravel() - np.asarray(want, F32).ravel())
    bound = 0.05 * n_steps * lr
    frac = float(np.mean(diff > bound))
    print("ADAMFRAC %s n=%d frac=%.3e maxdiff/klr=%.3f med/klr=%.5f" % (name, diff.size, frac, diff.max() / (n_steps * lr),
                                                                          np.median(diff) / (n_steps * lr)))
    assert frac <= max_frac, (name, "fraction beyond %.1e: %.2e" % (bound, frac), float(diff.max()))
    assert diff.max() <= 2.02 * n_steps * lr, (name, float(diff.max()))
    assert float(np.median(diff)) < 0.002 * n_steps * lr, (name, float(np.median(diff)))


def s_block_slices(eng):
    """what the S workgroups step or feed: W0[256:384, :], b0, the domain table"""
    w0 = eng.segments["W0"][0]
    out = {"W0[256:384]": slice(w0 + 256 * 256, w0 + 384 * 256)}
    for name in ("b0", "domain_emb"):
        off, cnt = eng.segments[name]
        out[name] = slice(off, off + cnt)
    return out


# ------------------------------------------------------------------ the S block from the live parameters
S_CASES = [(D, rows, None) for D in (1, 10, 17, 33) for rows in (1, 5, 1024)] + [(33, 1024, "mixed")]


@pytest.mark.parametrize("n_domain,rows,col", S_CASES, ids=["D%d-b%d%s" % (D, r, "-mixed" if c else "") for D, r, c in S_CASES])
def test_s_block_reads_live_parameters(env, n_domain, rows, col):
    """k_wgrad_adam's S workgroups take the pre-update W0[256:384, their 8 columns] from the live parameters, the block
    they step themselves later in the launch.  Against k_wgrad -> slabs -> k_update (MAMDR_FUSED=0), which keeps its
    snapshot: one SGD step at lr 1 (= the gradient) within rtol 2e-4 / atol 2e-6 x the largest gradient element, then
    three Adam steps within the multi-step Adam bar -- on W0[256:384], b0 and the domain table each."""
    d = n_domain - 1 if col is None else 0          # (the last domain: the highest row of the last one-hot block)
    params, data = make_inputs(n_domain, {d: (3 * rows, col)}, seed=11)
    grads, steps, slices = {}, {}, None
    for mode, fused in (("fused", "2"), ("slabs", "0")):
        eng = make_engine(env, n_domain, rows, params, data, switches={"MAMDR_FUSED": fused})
        assert int(eng.lib.mamdr_step_path(eng.ctx, rows)) == (1 if mode == "fused" else 0)
        slices = s_block_slices(eng)
        w0 = eng.get_weights()
        eng.train_steps(d, first_step=0, n_steps=1, lr=1.0, optimizer="sgd")
        grads[mode] = host(w0 - eng.get_weights())
        eng.set_weights(w0)
        eng.train_steps(d, first_step=0, n_steps=3, lr=1e-3)
        steps[mode] = host(eng.get_weights())
        eng.close()
    ga, gb = grads["fused"], grads["slabs"]
    atol = 2e-6 * max(np.abs(gb).max(), 1e-3)
    for name, sl in slices.items():
        assert np.abs(gb[sl]).max() > 0, name
        err = np.abs(ga[sl] - gb[sl])
        print("GRAD %s max|err|=%.3e atol=%.3e max|g|=%.3e" % (name, err.max(), atol, np.abs(gb[sl]).max()))
        np.testing.assert_allclose(ga[sl], gb[sl], rtol=2e-4, atol=atol, err_msg=name)
        assert_adam_close(steps["fused"][sl], steps["slabs"][sl], 3, 1e-3, name)


def test_accumulate_reads_the_same_block(env):
    """MAMDR_OPT_ACCUMULATE steps nothing, so the live read is the pre-update value trivially: the accumulator (from zero)
    holds the gradient an SGD step at lr 1 on the same batch applies, bit for bit -- p' = fl(p - g) for every element
    (dropout 0: the meta pass runs without it; two one-hot blocks, mixed domains)."""
    params, data = make_inputs(17, {0: (1024, "mixed")}, seed=12)
    eng = make_engine(env, 17, 1024, params, data, dropout=0.0)
    assert int(eng.lib.mamdr_step_path(eng.ctx, 1024)) == 1
    acc = eng.new_vector()
    eng.bind_accumulator(acc)
    w0 = host(eng.get_weights())
    eng.train_steps(0, first_step=0, n_steps=1, lr=1.0, optimizer="accumulate")
    assert same_bits(host(eng.get_weights()), w0)
    g = host(acc)
    eng.train_steps(0, first_step=0, n_steps=1, lr=1.0, optimizer="sgd")
    w1 = host(eng.get_weights())
    eng.close()
    for name, sl in list(s_block_slices(eng).items()) + [("all", slice(None))]:
        assert np.abs(g[sl]).max() > 0, name
        assert same_bits(w1[sl], (w0[sl] - g[sl]).astype(F32)), (name, int((w1[sl] != (w0[sl] - g[sl]).astype(F32)).sum()))


# ------------------------------------------------------------------ W1^T is never missed
def _three_calls(eng):
    """three rounds of (a pass of 5 rows, a pass of 1,024 + 1 rows), an outer update between them: every call starts from
    stale transposed copies"""
    for _ in range(3):
        eng.train_steps(0, lr=1e-3)
        eng.train_steps(1, lr=1e-3)
        eng.set_weights(eng.get_weights() * 0.9 + 1e-3)
    return state(eng)


def test_w1t_skipped_only_where_nothing_reads_it(env):
    """A context whose every k_tower4 launch takes the W1 image keeps no W1^T at all; one whose towers stream W1 / W1^T
    (MAMDR_T4_NO_W1L=1) reads the copy k_wgrad_adam keeps.  Same arithmetic either way: weights and both Adam slots
    agree bit for bit."""
    params, data = make_inputs(10, {0: (5, None), 1: (1025, None)}, seed=13)
    res = {}
    for mode in ("image", "stream"):
        eng = make_engine(env, 10, 1024, params, data, switches={"MAMDR_T4_NO_W1L": "1" if mode == "stream" else "0"})
        assert int(eng.lib.mamdr_step_path(eng.ctx, 1024)) == 1 and eng.tower_tile(1024) == 4
        res[mode] = _three_calls(eng)
        eng.close()
    for a, b, name in zip(res["image"], res["stream"], ("weights", "adam_m", "adam_v")):
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        assert same_bits(a, b), (name, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def test_streaming_tower_on_the_fused_path_finds_w1t(env):
    """MAMDR_FUSED=2 with four-row tiles at 2,048 rows: two rounds of workgroups, so k_tower4 streams W1^T on the
    k_wgrad_adam path and the steps after a call's first rely on the copy k_wgrad_adam keeps.  Against the same steps as
    one call each with the live state handed out in between (which drops the copies: every call transposes afresh):
    identical bits."""
    params, data = make_inputs(10, {3: (3 * 2048, None)}, seed=14)
    res = {}
    for mode in ("one_call", "three_calls"):
        eng = make_engine(env, 10, 2048, params, data, switches={"MAMDR_FUSED": "2"}, tower_tile=4)
        assert int(eng.lib.mamdr_step_path(eng.ctx, 2048)) == 1 and eng.tower_tile(2048) == 4
        if mode == "one_call":
            eng.train_steps(3, first_step=0, n_steps=3, lr=1e-3)
        else:
            for s in range(3):
                eng.train_steps(3, first_step=s, n_steps=1, lr=1e-3)
                eng.sync()
        res[mode] = state(eng)
        eng.close()
    for a, b, name in zip(res["one_call"], res["three_calls"], ("weights", "adam_m", "adam_v")):
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        assert same_bits(a, b), (name, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


# ------------------------------------------------------------------ every element is stored exactly once
STORE_SEED = 15     # (checked with the oracle: no dense element's gradient is zero -- the test asserts it again)


def centre_units(params, c):
    """biases := minus the per-unit median of the batch's pre-activations, layer by layer: every relu unit is active on half
    of the rows (with the initialiser's biases a few units of h2 / h3 are dead for a whole batch, whatever the seed)"""
    h = otower.gather(params, c["uid"], c["pid"], c["domain"])
    for l in range(3):
        z = h @ params["W%d" % l]
        params["b%d" % l] = (-np.median(z, axis=0)).astype(F32)
        h = np.maximum(z + params["b%d" % l], 0).astype(F32)


def test_every_dense_element_is_stored_once(env):
    """One Adam step from m = v = 0 on a batch whose gradient is non-zero in EVERY dense element (dropout 0, 256 rows,
    every domain and both labels, every relu unit active on half of the rows; the oracle confirms it):
    afterwards no element of p has its initial bits and no element of m or v is zero -- no hole in k_wgrad_adam's stores --
    and a second engine on the same inputs gives identical bits (no element stored twice with different values)."""
    D, rows = 10, 256
    params, data = make_inputs(D, {0: (rows, "mixed")}, seed=STORE_SEED)
    c = data[0]
    centre_units(params, c)
    assert set(c["domain"]) == set(range(D)) and set(c["label"]) == {0.0, 1.0}
    _, grads, _ = otower.loss_and_grads(params, c["uid"], c["pid"], c["domain"], c["label"], None, 0.0, False)
    runs = []
    for _ in range(2):
        eng = make_engine(env, D, rows, params, data, dropout=0.0)
        assert int(eng.lib.mamdr_step_path(eng.ctx, rows)) == 1
        w0 = host(eng.get_weights())
        eng.train_steps(0, first_step=0, n_steps=1, lr=1e-3)
        w1, m1, v1 = state(eng)
        for name, (off, cnt) in eng.segments.items():
            assert np.all(np.abs(grads[name]) > 1e-12), (name, "the oracle's gradient has a zero: choose another seed")
            sl = slice(off, off + cnt)
            assert not np.any(w1[sl].view(np.uint32) == w0[sl].view(np.uint32)), (name, "p not stored")
            assert not np.any(m1[sl] == 0), (name, "m not stored")
            assert not np.any(v1[sl] == 0), (name, "v not stored")
        runs.append((w1, m1, v1))
        eng.close()
    for a, b, name in zip(runs[0], runs[1], ("weights", "adam_m", "adam_v")):
        assert same_bits(a, b), name
