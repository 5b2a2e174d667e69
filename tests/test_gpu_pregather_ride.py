"""Rider workgroups of k_wgrad_adam gather the NEXT pass window (mamdr_pregather_ahead) while the current window's steps
run; mamdr_pregather_passes with the same list adopts what they gathered and launches k_pass_prep_multi over the rest.

Every case is a script of hints and passes run through the C ABI on engines of this file's own (64-row tables, 4 domains
of 2,048 rows, batch 1,024, dropout 0.5), once with riders and once with MAMDR_NO_PREGATHER_RIDE=1: weights and both Adam
slots agree bit for bit, and the counters show that the riders really gathered rows (a device without idle CUs -- no
riders -- fails these tests: they are about the riders).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import tower as otower      # noqa: E402

F32 = np.float32
N_USER = N_ITEM = 64
D, SPLIT, BATCH = 4, 2048, 1024
ROWS6 = (5, 1025, 37, 2048, 1, 1024)     # steps of 1 and 5 rows, a pass shorter than its 16 padding rows, slices across passes
PAD = 16


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine
    return engine


@pytest.fixture(scope="module")
def inputs():
    rs = np.random.RandomState(21)
    params = otower.init_params(rs, N_USER, N_ITEM, D)
    params["domain_emb"] = (rs.standard_normal(params["domain_emb"].shape) * 0.05).astype(F32)

    def columns():
        return [{"uid": rs.randint(0, N_USER, SPLIT).astype(np.int32), "pid": rs.randint(0, N_ITEM, SPLIT).astype(np.int32),
                 "domain": np.full(SPLIT, d, np.int32), "label": rs.permutation(np.arange(SPLIT) % 2).astype(F32)}
                for d in range(D)]
    data, other = columns(), columns()
    perms = [rs.permutation(SPLIT).astype(np.int32) for _ in range(24)]
    return params, data, other, perms


def window(rows, first_perm, domains=None):
    """[(domain, perm index, rows)]: pass k over domain k % D (or domains[k]) with a permutation of its own"""
    return [((domains[k] if domains else k % D), first_perm + k, r) for k, r in enumerate(rows)]


def positions(win):
    return sum(r + PAD for _, _, r in win if r > 0)


def steps(win):
    return sum(-(-r // BATCH) for _, _, r in win)


def run_script(engine, inputs, script, ride, profile=False):
    """script: ("hint", window) | ("ahead", window, spread_steps) | ("pass", (domain, perm index, rows)[, with_loss]) |
    ("rebind", domain).  -> (weights, adam_m, adam_v, losses), counters"""
    params, data, other, perms = inputs
    if not ride:
        os.environ["MAMDR_NO_PREGATHER_RIDE"] = "1"
    try:
        eng = engine.TowerEngine(N_USER, N_ITEM, D, BATCH, dropout=0.5)
    finally:
        os.environ.pop("MAMDR_NO_PREGATHER_RIDE", None)
    eng.bind_table("user_emb", params["user_emb"])
    eng.bind_table("item_emb", params["item_emb"])
    for d in range(D):
        c = data[d]
        eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
    eng.set_weights(eng.pack(params))
    assert int(eng.lib.mamdr_step_path(eng.ctx, BATCH)) == 1
    if profile:
        eng.profile(True)
    dev = [torch.from_numpy(p).to(eng.device) for p in perms]
    losses = torch.zeros(64, dtype=torch.float32, device=eng.device)
    n_loss = 0

    def listed(win):
        return [(d, None if k is None else dev[k], r) for d, k, r in win]
    for act in script:
        if act[0] == "hint":
            eng.pregather(listed(act[1]), BATCH)
        elif act[0] == "ahead":
            eng.pregather_ahead(listed(act[1]), BATCH, spread_steps=act[2])
        elif act[0] == "pass":
            d, k, r = act[1]
            n = -(-r // BATCH)
            out = None
            if len(act) > 2 and act[2] and n:
                out, n_loss = losses[n_loss:n_loss + n], n_loss + n
            eng.train_steps(d, perm=None if k is None else dev[k], lr=1e-3, pass_rows=r, loss_out=out)
        elif act[0] == "rebind":
            c = other[act[1]]
            eng.bind_domain_data(act[1], "train", c["uid"], c["pid"], c["domain"], c["label"])
        else:
            raise ValueError(act)
    state = [t.cpu().numpy().copy() for t in (eng.get_weights(), eng.adam_m, eng.adam_v, losses)]
    counters = {k: int(getattr(eng.lib, "mamdr_pregather_" + k)(eng.ctx)) for k in ("hits", "launches", "rider_rows", "remainder_rows")}
    eng.close()
    return state, counters


def windows_script(wins, with_loss=False):
    """the caller's protocol: hint the current window, announce the next one, run the current one's passes"""
    script = []
    for k, w in enumerate(wins):
        script.append(("hint", w))
        if k + 1 < len(wins):
            script.append(("ahead", wins[k + 1], steps(w)))
        script += [("pass", p, with_loss) for p in w]
    return script


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def assert_same(got, want, what):
    for a, b, name in zip(got, want, ("weights", "adam_m", "adam_v", "losses")):
        assert np.isfinite(a).all(), (what, name)
        assert same_bits(a, b), (what, name, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
    assert np.abs(got[1]).max() > 0 and np.abs(got[2]).max() > 0, what


def both(env, inputs, script):
    rode, c_ride = run_script(env, inputs, script, ride=True)
    plain, c_plain = run_script(env, inputs, script, ride=False)
    print("COUNTERS ride %s | no ride %s" % (c_ride, c_plain))
    assert_same(rode, plain, "riders vs MAMDR_NO_PREGATHER_RIDE=1")
    assert c_plain["rider_rows"] == 0 and c_plain["remainder_rows"] == 0
    assert c_ride["rider_rows"] > 0, "the riders gathered nothing"
    assert c_ride["hits"] == c_plain["hits"] and c_ride["launches"] == c_plain["launches"]
    return c_ride


def test_three_windows_of_mixed_passes(env, inputs):
    wins = [window(ROWS6, 6 * k) for k in range(3)]
    c = both(env, inputs, windows_script(wins))
    # both adopted windows were gathered once: by riders, the rest by the remainder launches
    assert c["rider_rows"] + c["remainder_rows"] == 2 * positions(wins[0])


def test_window_larger_than_the_riders_reach(env, inputs):
    """two steps carry at most 2 x 32 riders x 64 positions: the rest of the 8,256 is gathered by the remainder launch"""
    wins = [window((1024, 1024), 0), window((2048, 2048, 2048, 2048), 2)]
    assert positions(wins[1]) > steps(wins[0]) * 32 * 64
    c = both(env, inputs, windows_script(wins))
    assert c["remainder_rows"] > 0
    assert c["rider_rows"] + c["remainder_rows"] == positions(wins[1])


def test_spread_over_one_step(env, inputs):
    wins = [window((5,), 0), window(ROWS6, 1)]
    assert steps(wins[0]) == 1
    c = both(env, inputs, windows_script(wins))
    assert c["rider_rows"] + c["remainder_rows"] == positions(wins[1])


def test_empty_pass_inside_the_ahead_window(env, inputs):
    wins = [window(ROWS6, 0), window((37, 0, 1025, 0, 5), 6)]
    c = both(env, inputs, windows_script(wins))
    assert c["rider_rows"] + c["remainder_rows"] == positions(wins[1])


def test_passes_without_a_permutation(env, inputs):
    wins = [[(d, None, r) for d, _, r in window(ROWS6, 0)], [(d, None, r) for d, _, r in window(ROWS6[::-1], 0)]]
    c = both(env, inputs, windows_script(wins))
    assert c["rider_rows"] + c["remainder_rows"] == positions(wins[1])


def test_leaving_the_announced_order_drops_the_hint(env, inputs):
    """an unannounced pass between the announced ones: the window the riders were working on is dropped, the later hint
    gathers all of its window itself"""
    w0, w1 = window(ROWS6, 0), window(ROWS6, 6)
    script = [("hint", w0), ("ahead", w1, steps(w0))] + [("pass", p) for p in w0[:3]] + [("pass", (3, 20, 37))] + \
             [("pass", p) for p in w0[3:]] + [("hint", w1)] + [("pass", p) for p in w1]
    c = both(env, inputs, script)
    assert 0 < c["rider_rows"] <= positions(w1) and c["remainder_rows"] == 0


def test_steps_that_report_their_loss_carry_one_rider_fewer(env, inputs):
    wins = [window(ROWS6, 0), window(ROWS6, 6)]
    c = both(env, inputs, windows_script(wins, with_loss=True))
    assert c["rider_rows"] + c["remainder_rows"] == positions(wins[1])


def test_rebound_columns_drop_what_the_riders_gathered(env, inputs):
    """mamdr_bind_domain_data between the announcement and the adoption: the rows gathered from the old columns are not
    used (both runs train the second window on the new columns)"""
    w0, w1 = window(ROWS6, 0), window(ROWS6, 6)
    script = [("hint", w0), ("ahead", w1, steps(w0))] + [("pass", p) for p in w0] + [("rebind", 1), ("hint", w1)] + \
             [("pass", p) for p in w1]
    c = both(env, inputs, script)
    assert c["rider_rows"] > 0 and c["remainder_rows"] == 0
    # ... and the new columns matter: the same script without the rebind ends elsewhere
    kept, _ = run_script(env, inputs, [a for a in script if a[0] != "rebind"], ride=True)
    rebound, _ = run_script(env, inputs, script, ride=True)
    assert not same_bits(kept[0], rebound[0])


def test_profiled_context_rides_nothing(env, inputs):
    wins = [window(ROWS6, 6 * k) for k in range(2)]
    script = windows_script(wins)
    both(env, inputs, script)
    prof, c = run_script(env, inputs, script, ride=True, profile=True)
    plain, _ = run_script(env, inputs, script, ride=False)
    assert c["rider_rows"] == 0 and c["remainder_rows"] == 0
    assert_same(prof, plain, "profile mode")
