"""k_tower4 on a pre-gathered pass: every wave fetches its own slice of the x tile and, with the domain-table step pending
on a one-domain tile (`same`), starts layer 0 with no workgroup barrier in front of it.

The yardstick in every case is the path that change does not touch: the same run with MAMDR_NO_PREGATHER=1, where the
tower gathers its rows itself through the shared LDS tile and both barriers (tests/test_gpu_parity.py holds that switch
to "bit-identical").  Only who fetches x and who waits for whom differs -- the A values, the B values and the order of
every MFMA and every LDS sum do not -- so weights, Adam m, Adam v and the per-step losses must agree as uint32 bits.
Every case runs twice on either path (`check`): a call that reports its per-step losses materialises the pending
domain-table step before every step, so the barrier-free start (`same`) only happens in the run WITHOUT losses and shows
in the weights and Adam slots it leaves; the run with losses holds the fallback to the same bits.

The engines are built on small problems of this file's own (engine.TowerEngine directly, 64 users / 64 items); every
engine is asserted to be on the k_wgrad_adam path with four-row tiles, so no case can silently run another kernel.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import tower as otower      # noqa: E402

F32 = np.float32
N_USER = N_ITEM = 64
NAMES = ("weights", "adam_m", "adam_v", "losses")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine
    return engine


def make_inputs(n_domain, splits, seed):
    """parameters, frozen tables and the train splits.  splits: {domain id the split is bound under: (rows, domain column)},
    the column None = that id itself, "mixed" = every domain id in turn (shuffled), an int = that constant id."""
    rs = np.random.RandomState(seed)
    params = otower.init_params(rs, N_USER, N_ITEM, n_domain)
    params["domain_emb"] = (rs.standard_normal(params["domain_emb"].shape) * 0.05).astype(F32)
    for l in range(3):
        params["b%d" % l] = (rs.standard_normal(params["b%d" % l].shape) * 0.05).astype(F32)
    data = {}
    for d, (rows, col) in splits.items():
        if col is None:
            dom = np.full(rows, d, np.int32)
        elif isinstance(col, str):      # "mixed"
            dom = rs.permutation(np.arange(rows) % n_domain).astype(np.int32)
        elif callable(col):
            dom = np.asarray(col(rows), np.int32)
        else:
            dom = np.full(rows, col, np.int32)
        data[d] = {"uid": rs.randint(0, N_USER, rows).astype(np.int32), "pid": rs.randint(0, N_ITEM, rows).astype(np.int32),
                   "domain": dom, "label": rs.permutation(np.arange(rows) % 2).astype(F32)}
    return params, data


def make_engine(engine, n_domain, batch, params, data, dropout, switches):
    """(the library reads its switches when the context is created)"""
    os.environ.update(switches)
    try:
        eng = engine.TowerEngine(N_USER, N_ITEM, n_domain, batch, dropout=dropout)
    finally:
        for k in switches:
            os.environ.pop(k, None)
    eng.bind_table("user_emb", params["user_emb"])
    eng.bind_table("item_emb", params["item_emb"])
    for d, c in data.items():
        eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
    eng.set_weights(eng.pack(params))
    assert int(eng.lib.mamdr_step_path(eng.ctx, batch)) == 1 and eng.tower_tile(batch) == 4
    return eng


def host(t):
    return t.cpu().numpy().copy()


def run(engine, n_domain, batch, params, data, script, dropout=0.5, pregather=True, switches=None, want_losses=False):
    """script: ("train", domain, n_steps or None) | ("window", [domains]) | ("assign",).  -> weights, Adam m, Adam v and, with
    want_losses, the loss of every step in order.  A call that reports its losses materialises the domain-table step
    before every step (the reported loss reads the tables), so such a run never has a step pending: the pending path
    shows in the run without losses, through the weights and both Adam slots."""
    sw = dict(switches or {})
    sw["MAMDR_NO_PREGATHER"] = "0" if pregather else "1"
    eng = make_engine(engine, n_domain, batch, params, data, dropout, sw)
    losses = []
    for op in script:
        if op[0] == "train":
            n_steps = op[2] if op[2] is not None else -(-eng.n_rows(op[1], "train") // batch)
            out = torch.zeros(n_steps, dtype=torch.float32, device=eng.device) if want_losses else None
            eng.train_steps(op[1], first_step=0, n_steps=n_steps, lr=1e-3, loss_out=out)
            if want_losses:
                losses.append(host(out))
        elif op[0] == "window":           # the passes of the next calls, gathered in one launch (a no-op without pre-gather)
            eng.pregather([(d, None) for d in op[1]])
        else:                             # an outer update between calls: the pending domain-table step is materialised
            eng.set_weights(eng.get_weights() * 0.9 + 1e-3)
    res = (host(eng.get_weights()), host(eng.adam_m), host(eng.adam_v))
    if want_losses:
        res += (np.concatenate(losses),)
    eng.close()
    return res


def assert_same_bits(got, want, what):
    for a, b, name in zip(got, want, NAMES):
        assert a.shape == b.shape, (what, name)
        assert np.isfinite(a).all() and np.abs(a).max() > 0, (what, name)
        au, bu = np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32)
        assert np.array_equal(au, bu), (what, name, "%d of %d elements differ" % (int((au != bu).sum()), au.size))


def check(engine, n_domain, batch, splits, script, seed, dropout=0.5, switches=None):
    """the script twice on either path: without losses (the domain-table step stays pending from step to step) and with
    them (never pending: every step takes the fallback with both barriers)"""
    params, data = make_inputs(n_domain, splits, seed)
    out = {}
    for want_losses in (False, True):
        new = run(engine, n_domain, batch, params, data, script, dropout, True, switches, want_losses)
        ref = run(engine, n_domain, batch, params, data, script, dropout, False, switches, want_losses)
        assert_same_bits(new, ref, "pre-gathered vs MAMDR_NO_PREGATHER=1, %s losses" % ("with" if want_losses else "without"))
        out[want_losses] = new
    return out


# ------------------------------------------------------------------ row counts: the slice and its zeroing
@pytest.mark.parametrize("dropout", [0.5, 0.0], ids=["drop.5", "drop0"])
@pytest.mark.parametrize("batch", [1, 3, 4, 5, 7, 1024])
def test_row_counts(env, batch, dropout):
    """3 steps of `batch` rows: steps 2 and 3 run with the domain-table step pending (`same` true).  The grid covers the
    rows padded to 16, so at 5 / 7 rows the second tile has 1 / 3 valid rows and the tiles behind it are all padding; at
    1 / 3 rows the first tile is partly padding."""
    check(env, 10, batch, {3: (3 * batch, None)}, [("train", 3, 3)], seed=21, dropout=dropout)


@pytest.mark.parametrize("dropout", [0.5, 0.0], ids=["drop.5", "drop0"])
def test_full_step_then_one_row_step(env, dropout):
    """a pass of 1,024 + 1 rows, twice: a full step, a one-row step (255 tiles of padding behind one row), and the same
    again with the step pending from the call before"""
    check(env, 10, 1024, {3: (1025, None)}, [("train", 3, None), ("train", 3, None)], seed=22, dropout=dropout)


# ------------------------------------------------------------------ the fallbacks without `same`: both barriers stay
@pytest.mark.parametrize("n_domain", [1, 10, 17])
@pytest.mark.parametrize("rows", [5, 256])
def test_mixed_domains_in_a_tile(env, rows, n_domain):
    """every domain id in turn: the tiles hold several domains, the domain columns go through LDS across waves"""
    check(env, n_domain, rows, {0: (3 * rows, "mixed")}, [("train", 0, 3)], seed=23)


@pytest.mark.parametrize("n_domain", [10, 17])
@pytest.mark.parametrize("rows", [5, 256])
def test_hint_mismatch(env, rows, n_domain):
    """a split bound under domain id 2 whose domain column holds the constant id n_domain - 1: one domain per tile, but not
    the one the caller announced"""
    check(env, n_domain, rows, {2: (3 * rows, n_domain - 1)}, [("train", 2, 3)], seed=24)


def _odd_row_per_tile(rows):
    """the announced domain 2 everywhere, but in tile t of every 16-row step row t & 3 holds domain 5"""
    dom = np.full(rows, 2, np.int32)
    dom[np.arange(rows) % 16 % 5 == 0] = 5          # positions 0, 5, 10, 15 of a step: rows 0, 1, 2, 3 of tiles 0, 1, 2, 3
    return dom


def _odd_last_row(rows):
    """steps of 5 rows whose last row -- row 0 of the second tile, whose padding rows take its (clamped) domain -- holds
    domain 5: the first tile has `same`, the others do not"""
    dom = np.full(rows, 2, np.int32)
    dom[np.arange(rows) % 5 == 4] = 5
    return dom


@pytest.mark.parametrize("batch,col", [(16, _odd_row_per_tile), (5, _odd_last_row)], ids=["odd-row-per-tile", "odd-last-row"])
def test_each_row_takes_part_in_the_same_decision(env, batch, col):
    """one row of a tile differs from the announced domain, at each of the four positions in turn: a decision that
    overlooked that row would hand it the announced domain's embedding.  Tiles with and without `same` in one launch."""
    check(env, 10, batch, {2: (3 * batch, col)}, [("train", 2, 3)], seed=30)


@pytest.mark.parametrize("n_domain", [1, 10, 17])
@pytest.mark.parametrize("rows", [5, 1024])
def test_first_step_of_a_fresh_context(env, rows, n_domain):
    """nothing pending: one step, one call"""
    check(env, n_domain, rows, {n_domain - 1: (rows, None)}, [("train", n_domain - 1, 1)], seed=25)


@pytest.mark.parametrize("n_domain", [1, 17])
def test_pending_step_at_other_domain_counts(env, n_domain):
    """`same` at 1 and 17 domains (test_row_counts runs 10): the workgroups below the domain count write a domain row back"""
    check(env, n_domain, 5, {n_domain - 1: (15, None)}, [("train", n_domain - 1, 3)], seed=26)


# ------------------------------------------------------------------ both pre-gathered instances
@pytest.mark.parametrize("rows", [5, 1025])
def test_streaming_instance(env, rows):
    """MAMDR_T4_NO_W1L=1: the instance that streams W1 / W1^T, on the k_wgrad_adam path over pre-gathered rows"""
    check(env, 10, 1024, {1: (rows, None)}, [("train", 1, None), ("train", 1, None), ("train", 1, None)], seed=27,
          switches={"MAMDR_T4_NO_W1L": "1"})


# ------------------------------------------------------------------ across calls and windows
def test_pending_across_calls_and_windows(env):
    """three rounds of (a pass over domain 0 of 5 rows, a pass over domain 1 of 1,024 + 1 rows) with an outer update in
    between: a window holds two passes, the domain step stays pending from one call to the next, and the hint changes
    with the pass"""
    script = []
    for _ in range(3):
        script += [("window", [0, 1]), ("train", 0, None), ("train", 1, None), ("assign",)]
    check(env, 10, 1024, {0: (5, None), 1: (1025, None)}, script, seed=28)


# ------------------------------------------------------------------ determinism
def test_two_engines_same_bits(env):
    """no barrier in front of layer 0 must not open a race: two engines on the same inputs give identical bits"""
    params, data = make_inputs(10, {0: (5, None), 1: (1025, None), 2: (256, "mixed")}, seed=29)
    script = [("train", 1, None), ("train", 0, None), ("train", 2, None), ("train", 1, None)]
    a = run(env, 10, 1024, params, data, script)
    b = run(env, 10, 1024, params, data, script)
    assert_same_bits(a, b, "two engines")
