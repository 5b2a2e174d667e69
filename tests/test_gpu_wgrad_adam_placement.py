"""Which workgroup of k_wgrad_adam computes which block, and whether the towers read W2 or its transposed copy, are
speed choices: neither may show in a single bit of the result.

* MAMDR_FZ_S_INORDER=1 deals the S workgroups their 8-column blocks of dz1 in grid order instead of by XCD
  (mamdr_amd/csrc/wgrad_adam_deal.h).  Every value is a function of the block, not of the workgroup.
* MAMDR_NO_W2_DIRECT=1 builds k_tower4's transposed copies at the start of a call and has k_wgrad_adam keep W2^T current;
  without it a context whose every tower can read W2 in place keeps no copy at all.

Small engines of this file's own, built as in tests/test_gpu_param_handoff.py (64 users / items, dropout 0.5)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import tower as otower      # noqa: E402

F32 = np.float32
N_USER = N_ITEM = 64
NAMES = ("weights", "adam_m", "adam_v")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine
    return engine


def make_inputs(n_domain, passes, seed):
    """parameters, frozen tables and the train splits {domain id: columns}; passes: {domain id: (rows, domain column:
    None = the domain id itself, "mixed" = every domain id in turn, shuffled)}"""
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


def make_engine(engine, n_domain, batch, params, data, switches):
    """(the library reads its switches when the context is created)"""
    os.environ.update(switches)
    try:
        eng = engine.TowerEngine(N_USER, N_ITEM, n_domain, batch, dropout=0.5)
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


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def raw_state(eng):
    """the bound vectors as the launches left them: no mamdr_sync_tables (the domain table's last step still pending)"""
    torch.cuda.synchronize()
    return host(eng._weights), host(eng._adam_m), host(eng._adam_v)


def synced_state(eng):
    eng.sync()
    return raw_state(eng)


def assert_same_state(a, b, what, sl=slice(None)):
    for x, y, name in zip(a, b, NAMES):
        assert np.isfinite(x[sl]).all(), (what, name)
        diff = int((x[sl].view(np.uint32) != y[sl].view(np.uint32)).sum())
        assert same_bits(x[sl], y[sl]), (what, name, "%d elements differ" % diff)


# 5 rows: one ragged 16-row tile, seven of the eight wave shares empty; 17 domains: two one-hot blocks; mixed: the towers'
# per-lane domain path and every row of both one-hot blocks
PLACEMENT_CASES = [(1, 5, None), (17, 5, None), (17, 64, None), (17, 64, "mixed")]


@pytest.mark.parametrize("n_domain,rows,col", PLACEMENT_CASES,
                         ids=["D%d-b%d%s" % (D, r, "-mixed" if c else "") for D, r, c in PLACEMENT_CASES])
def test_s_placement_is_invisible(env, n_domain, rows, col):
    """Three Adam steps in two engines that differ only in MAMDR_FZ_S_INORDER: the dense block of the weights and both
    Adam slots agree bit for bit as the launches leave them, and after mamdr_sync_tables -- which applies the pending
    domain-table step from the 32 partial gradients pdm[blk] -- so does everything, the domain table included."""
    d = n_domain - 1 if col is None else 0
    params, data = make_inputs(n_domain, {d: (3 * rows, col)}, seed=21)
    raw, synced, seg = {}, {}, None
    for mode in ("dealt", "inorder"):
        eng = make_engine(env, n_domain, rows, params, data, switches={"MAMDR_FZ_S_INORDER": "1" if mode == "inorder" else "0"})
        assert int(eng.lib.mamdr_step_path(eng.ctx, rows)) == 1
        seg = dict(eng.segments)
        w0 = host(eng.get_weights())
        eng.train_steps(d, first_step=0, n_steps=3, lr=1e-3)
        # (bit 2 of the launch's flag word: the switch was read and reached the kernel)
        assert (int(eng.lib.mamdr_fused_flags(eng.ctx)) & 4 != 0) == (mode == "inorder")
        raw[mode] = raw_state(eng)
        synced[mode] = synced_state(eng)
        eng.close()
        # the steps moved what the S workgroups own: W0[256:384], b0 and (once synchronised) the domain table
        w = synced[mode][0]
        for name in ("W0", "b0", "domain_emb"):
            off, cnt = seg[name]
            lo = off + 256 * 256 if name == "W0" else off
            assert np.any(w[lo:off + cnt] != w0[lo:off + cnt]), (mode, name, "not stepped")
    dm_off, dm_cnt = seg["domain_emb"]
    assert dm_off == 0                          # (the domain table opens the dense block: everything behind it is `dense`)
    assert_same_state(raw["dealt"], raw["inorder"], "dense block before the sync", slice(dm_cnt, None))
    assert_same_state(synced["dealt"], synced["inorder"], "after mamdr_sync_tables")
    assert_same_state(synced["dealt"], synced["inorder"], "domain table", slice(dm_off, dm_off + dm_cnt))


def test_w2_read_in_place_matches_the_kept_copy(env):
    """10 domains, 64 rows per step, two engines that differ only in MAMDR_NO_W2_DIRECT, through the three ways a call can
    meet the W2 copy: (1) two Adam calls of three steps (the second starts from what the first left), (2) new weights
    assigned between two calls, (3) an accumulate call (no weight changes, no copy kept) followed by an Adam call.  After
    each, weights and both Adam slots agree bit for bit."""
    rows = 64
    params, data = make_inputs(10, {2: (6 * rows, None), 5: (6 * rows, "mixed")}, seed=22)
    engs = {mode: make_engine(env, 10, rows, params, data, switches={"MAMDR_NO_W2_DIRECT": "1" if mode == "copy" else "0"})
            for mode in ("inplace", "copy")}
    accs = {}
    for mode, eng in engs.items():
        assert int(eng.lib.mamdr_step_path(eng.ctx, rows)) == 1 and eng.tower_tile(rows) == 4
        accs[mode] = eng.new_vector()
        eng.bind_accumulator(accs[mode])

    def compare(what):
        st = {mode: synced_state(eng) for mode, eng in engs.items()}
        assert np.abs(st["inplace"][0]).max() > 0
        assert_same_state(st["inplace"], st["copy"], what)

    def flags():
        """bit 1 of the latest launch's flag word: every tower of its call read W2 in place and no copy was built or kept
        -- in the in-place engine only"""
        for mode, eng in engs.items():
            assert (int(eng.lib.mamdr_fused_flags(eng.ctx)) & 2 != 0) == (mode == "inplace"), mode

    try:
        w_start = {mode: host(eng.get_weights()) for mode, eng in engs.items()}
        for eng in engs.values():                                   # (1)
            eng.train_steps(2, first_step=0, n_steps=3, lr=1e-3)
            eng.train_steps(2, first_step=3, n_steps=3, lr=1e-3)
        flags()
        compare("two Adam calls")
        assert not same_bits(host(engs["inplace"].get_weights()), w_start["inplace"])
        for eng in engs.values():                                   # (2)
            eng.train_steps(5, first_step=0, n_steps=3, lr=1e-3)
            eng.set_weights(eng.get_weights() * 0.9 + 1e-3)
            eng.train_steps(5, first_step=3, n_steps=3, lr=1e-3)
        flags()
        compare("set_weights between two calls")
        for eng in engs.values():                                   # (3)
            eng.train_steps(2, first_step=0, n_steps=3, lr=1.0, optimizer="accumulate")
            eng.train_steps(2, first_step=3, n_steps=3, lr=1e-3)
        flags()
        compare("accumulate, then Adam")
        a, b = host(accs["inplace"]), host(accs["copy"])
        assert np.abs(a).max() > 0 and same_bits(a, b), "accumulators"
    finally:
        for eng in engs.values():
            eng.close()
