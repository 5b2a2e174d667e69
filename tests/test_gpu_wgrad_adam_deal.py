"""Which own workgroup of k_wgrad_adam computes which S block, tile or half of the output unit is a speed choice
(mamdr_amd/csrc/wgrad_adam_deal.h): the dealing by matrix, the default, and the residue dealing (MAMDR_FZ_DEAL_RESIDUE=1) must
not differ in a single bit of the result.

Two engines of this file's own per case (64 users / items, dropout 0.5, every domain id in the domain column so that each
one-hot block of the S workgroups meets samples) differ only in the switch; each takes three Adam steps and one SGD step.
Afterwards the whole bound vectors agree bit for bit -- the dense block and both Adam slots as the launches left them, and
after mamdr_sync_tables the domain table too -- and so does the loss where it was requested; bit 3 of mamdr_fused_flags
follows the switch and the steps ran on the fused path.

rows  1     one padded 16-row tile (seven of the eight wave shares empty)
rows  17    two 16-row tiles, the padding rows meet zero gradients
rows  1,024 the path's largest, with 10 domains (one one-hot block) and 33 (three: another LDS layout of the S workgroups)
loss        the step's loss requested: workgroup 242 behind the dealt ones
riders      a pass window announced: rider workgroups behind the own ones gather it.  The pre-gathered buffer has no
            accessor; the window's steps read their rows from it and from nowhere else, so what they leave is the check
            (and the rider counters, which must be equal and not zero)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import tower as otower      # noqa: E402

F32 = np.float32
N_USER = N_ITEM = 64
NAMES = ("weights", "adam_m", "adam_v")
SWITCH = "MAMDR_FZ_DEAL_RESIDUE"


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine
    return engine


def make_inputs(n_domain, n_rows, seed):
    rs = np.random.RandomState(seed)
    params = otower.init_params(rs, N_USER, N_ITEM, n_domain)
    params["domain_emb"] = (rs.standard_normal(params["domain_emb"].shape) * 0.05).astype(F32)
    for l in range(3):
        params["b%d" % l] = (rs.standard_normal(params["b%d" % l].shape) * 0.05).astype(F32)
    data = {"uid": rs.randint(0, N_USER, n_rows).astype(np.int32), "pid": rs.randint(0, N_ITEM, n_rows).astype(np.int32),
            "domain": rs.permutation(np.arange(n_rows) % n_domain).astype(np.int32),
            "label": rs.permutation(np.arange(n_rows) % 2).astype(F32)}
    return params, data


def make_engine(engine, n_domain, batch, params, data, residue):
    """(the library reads its switches when the context is created)"""
    os.environ[SWITCH] = "1" if residue else "0"
    try:
        eng = engine.TowerEngine(N_USER, N_ITEM, n_domain, batch, dropout=0.5)
    finally:
        os.environ.pop(SWITCH, None)
    eng.bind_table("user_emb", params["user_emb"])
    eng.bind_table("item_emb", params["item_emb"])
    eng.bind_domain_data(0, "train", data["uid"], data["pid"], data["domain"], data["label"])
    eng.set_weights(eng.pack(params))
    assert int(eng.lib.mamdr_step_path(eng.ctx, batch)) == 1
    return eng


def host(t):
    return t.cpu().numpy().copy()


def raw_state(eng):
    """the bound vectors as the launches left them: no mamdr_sync_tables (the domain table's last step still pending)"""
    torch.cuda.synchronize()
    return host(eng._weights), host(eng._adam_m), host(eng._adam_v)


def assert_same_bits(a, b, what):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    assert np.isfinite(a).all(), what
    diff = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    assert diff == 0, (what, "%d elements differ" % diff)


def compare(res, n_domain):
    """res: {mode: {"raw", "synced", "start", "seg", "loss"}}"""
    new, old = res["matrix"], res["residue"]
    dm_off, dm_cnt = new["seg"]["domain_emb"]
    assert dm_off == 0                          # (the domain table opens the dense block: everything behind it is `dense`)
    for x, y, name in zip(new["raw"], old["raw"], NAMES):
        assert_same_bits(x[dm_cnt:], y[dm_cnt:], "dense block before the sync: " + name)
    for x, y, name in zip(new["synced"], old["synced"], NAMES):
        assert_same_bits(x, y, "after mamdr_sync_tables: " + name)
        assert_same_bits(x[:dm_cnt], y[:dm_cnt], "domain table: " + name)
    if new["loss"] is not None:
        assert_same_bits(new["loss"], old["loss"], "reported loss")
        assert np.all(new["loss"] > 0)
    # the steps moved what every kind of workgroup owns
    w, w0 = new["synced"][0], new["start"]
    for name in ("W0", "b0", "W1", "b1", "W2", "b2", "wo", "gb", "domain_emb"):
        off, cnt = new["seg"][name]
        assert np.any(w[off:off + cnt] != w0[off:off + cnt]), (name, "not stepped")
    assert np.abs(new["synced"][1]).max() > 0 and np.abs(new["synced"][2]).max() > 0


def check_flags(eng, residue):
    """bit 3 of the launch's flag word: the switch was read and reached the kernel"""
    assert (int(eng.lib.mamdr_fused_flags(eng.ctx)) & 8 != 0) == residue


CASES = [(1, 10, False), (17, 10, False), (1024, 10, False), (1024, 33, False), (17, 33, True)]


@pytest.mark.parametrize("rows,n_domain,with_loss", CASES,
                         ids=["b%d-D%d%s" % (r, D, "-loss" if l else "") for r, D, l in CASES])
def test_the_dealing_is_invisible(env, rows, n_domain, with_loss):
    params, data = make_inputs(n_domain, 4 * rows, seed=31)
    res = {}
    for mode in ("matrix", "residue"):
        eng = make_engine(env, n_domain, rows, params, data, residue=mode == "residue")
        start = host(eng.get_weights())
        loss = torch.zeros(4, dtype=torch.float32, device=eng.device) if with_loss else None
        eng.train_steps(0, first_step=0, n_steps=3, lr=1e-3, loss_out=None if loss is None else loss[:3])
        check_flags(eng, mode == "residue")
        eng.train_steps(0, first_step=3, n_steps=1, lr=1e-2, optimizer="sgd", loss_out=None if loss is None else loss[3:])
        check_flags(eng, mode == "residue")
        raw = raw_state(eng)
        eng.sync()
        res[mode] = {"raw": raw, "synced": raw_state(eng), "start": start, "seg": dict(eng.segments),
                     "loss": None if loss is None else host(loss)}
        eng.close()
    compare(res, n_domain)


def test_the_dealing_is_invisible_with_riders_behind(env):
    """Window 0 is one pass of 2,048 rows (two Adam steps); window 1, announced before it runs, is a pass of 1,024 rows (an
    Adam step) and one of 37 (an SGD step).  The riders of window 0's two launches gather window 1 (1,093 positions with
    the padding rows; 14 idle CUs x 64 positions x 2 steps reach 1,792), and window 1's steps train on what they gathered."""
    rows, n_domain, pad = 1024, 10, 16
    params, data = make_inputs(n_domain, 2 * rows, seed=32)
    rs = np.random.RandomState(33)
    perms = [rs.permutation(2 * rows).astype(np.int32) for _ in range(3)]
    res, counters = {}, {}
    for mode in ("matrix", "residue"):
        eng = make_engine(env, n_domain, rows, params, data, residue=mode == "residue")
        start = host(eng.get_weights())
        dev = [torch.from_numpy(p).to(eng.device) for p in perms]
        w0, w1 = [(0, dev[0], 2 * rows)], [(0, dev[1], rows), (0, dev[2], 37)]
        eng.pregather(w0, rows)
        eng.pregather_ahead(w1, rows, spread_steps=2)
        eng.train_steps(0, perm=dev[0], lr=1e-3, pass_rows=2 * rows)
        check_flags(eng, mode == "residue")
        eng.pregather(w1, rows)
        eng.train_steps(0, perm=dev[1], lr=1e-3, pass_rows=rows)
        eng.train_steps(0, perm=dev[2], lr=1e-2, optimizer="sgd", pass_rows=37)
        check_flags(eng, mode == "residue")
        raw = raw_state(eng)
        eng.sync()
        res[mode] = {"raw": raw, "synced": raw_state(eng), "start": start, "seg": dict(eng.segments), "loss": None}
        counters[mode] = {k: int(getattr(eng.lib, "mamdr_pregather_" + k)(eng.ctx)) for k in ("hits", "launches", "rider_rows", "remainder_rows")}
        eng.close()
    print("COUNTERS", counters)
    assert counters["matrix"] == counters["residue"]
    assert counters["matrix"]["rider_rows"] > 0, "the riders gathered nothing"
    assert counters["matrix"]["rider_rows"] + counters["matrix"]["remainder_rows"] == rows + pad + 37 + pad
    compare(res, n_domain)
