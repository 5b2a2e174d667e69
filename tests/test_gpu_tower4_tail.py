"""k_tower4's W1-image instances behind layer 0: a wave's share of the image is requested AHEAD of the barriers that guard
the contractions' A operands (layer 1: behind t4_w1_landed(), in front of layer 0's exchange; backward 1: inside the
output-unit phase), and the output unit's dot product and the domain-table step's group sums exchange lanes on the vector
ALU (mamdr_amd/csrc/wave_exchange.h).

The yardstick is the streaming instance of the same launch (MAMDR_T4_NO_W1L=1): it runs the same split of k over the waves,
the same column ownership and the same slot sums as the image instance, and the moved reads do not touch its contraction
code.  YARDSTICK ESTABLISHED ON THE PARENT COMMIT (its library, this file's cases, an MI355X): image and streaming instance
agree bit for bit -- weights, Adam m, Adam v and the per-step losses of a three-step Adam call -- in every case below, for
the frozen-table mlp tower and for the DeepFM tower with trainable tables.  So the new image instance is held to the
streaming instance's bits.  (The C ABI does not expose `acts` / `dz`; whatever is wrong in them shows in the weight
gradients, i.e. in all three vectors after three steps.)

Cases, the smallest at which the moved reads can go wrong: 1, 4, 5, 64 and 257 rows per step (a partly padded tile, one full
tile, a tile behind a full one, 16 tiles, more than one tile per 16-row group with one valid row in the last); 10 domains,
and 33 domains on a 4-row batch (the grid's four tiles write the domain rows tile + 4, tile + 8, ... back in the small-grid
loop); a one-domain batch of the announced domain (`same`), a mixed-domain batch and a hint mismatch; a THREE-step call, so
that a domain-table step is pending in steps 2 and 3 of the run without losses (a call that reports its losses
materialises the step before every step: that run holds the fallback and the losses to the same bits).
"""
import os

import numpy as np
import pytest

import test_gpu_tower4_wave_start as ws

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
STREAMING = {"MAMDR_T4_NO_W1L": "1"}
ROWS = [1, 4, 5, 64, 257]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine
    return engine


def split_of(kind, rows, n_domain):
    """{domain id the split is bound under: (rows of three steps, domain column)} and that id"""
    if kind == "same":
        return {3: (3 * rows, None)}, 3
    if kind == "mixed":
        return {0: (3 * rows, "mixed")}, 0
    return {2: (3 * rows, n_domain - 1)}, 2          # one domain per tile, but not the announced one


# ------------------------------------------------------------------ the frozen-table mlp tower (k_wgrad_adam path)
def check_mlp(engine, n_domain, rows, kind, seed):
    splits, d = split_of(kind, rows, n_domain)
    params, data = ws.make_inputs(n_domain, splits, seed)
    script = [("train", d, 3)]
    for want_losses in (False, True):
        image = ws.run(engine, n_domain, rows, params, data, script, want_losses=want_losses)
        stream = ws.run(engine, n_domain, rows, params, data, script, switches=STREAMING, want_losses=want_losses)
        ws.assert_same_bits(image, stream, "W1 image vs MAMDR_T4_NO_W1L=1, %s losses" % ("with" if want_losses else "without"))


@pytest.mark.parametrize("kind", ["same", "mixed", "mismatch"])
@pytest.mark.parametrize("rows", ROWS)
def test_mlp_image_instance_has_the_streaming_instance_bits(env, rows, kind):
    check_mlp(env, 10, rows, kind, seed=41)


@pytest.mark.parametrize("kind", ["same", "mixed", "mismatch"])
def test_mlp_small_grid_writes_the_domain_rows_beyond_its_tiles(env, kind):
    """33 domains, 4 rows: four tiles, tile + n_tiles < n_domain -- every tile walks the small-grid loop"""
    check_mlp(env, 33, 4, kind, seed=42)


# ------------------------------------------------------------------ the DeepFM tower with trainable tables (DX / FM instance)
def run_deepfm(engine, n_domain, rows, params, data, d, switches, want_losses):
    os.environ.update(switches)
    try:
        eng = engine.TowerEngine(ws.N_USER, ws.N_ITEM, n_domain, rows, dropout=0.5, emb_trainable=True, tower="deepfm")
    finally:
        for k in switches:
            os.environ.pop(k, None)
    c = data[d]
    eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
    eng.set_weights(eng.pack(params))
    assert eng.tower_tile(rows) == 4
    out = torch.zeros(3, dtype=torch.float32, device=eng.device) if want_losses else None
    eng.train_steps(d, first_step=0, n_steps=3, lr=1e-3, loss_out=out)
    res = (ws.host(eng.get_weights()), ws.host(eng.adam_m), ws.host(eng.adam_v))
    if want_losses:
        res += (ws.host(out),)
    eng.close()
    return res


def check_deepfm(engine, n_domain, rows, kind, seed):
    splits, d = split_of(kind, rows, n_domain)
    params, data = ws.make_inputs(n_domain, splits, seed)
    rs = np.random.RandomState(seed + 1000)          # non-zero linear tables: every term of the logit is exercised
    params["lin_domain"] = (rs.standard_normal(n_domain) * 0.05).astype(F32)
    params["lin_user"] = (rs.standard_normal(ws.N_USER) * 0.05).astype(F32)
    params["lin_item"] = (rs.standard_normal(ws.N_ITEM) * 0.05).astype(F32)
    for want_losses in (False, True):
        image = run_deepfm(engine, n_domain, rows, params, data, d, {}, want_losses)
        stream = run_deepfm(engine, n_domain, rows, params, data, d, STREAMING, want_losses)
        ws.assert_same_bits(image, stream, "deepfm, W1 image vs MAMDR_T4_NO_W1L=1, %s losses" % ("with" if want_losses else "without"))


@pytest.mark.parametrize("kind", ["same", "mixed"])
@pytest.mark.parametrize("rows", ROWS)
def test_deepfm_image_instance_has_the_streaming_instance_bits(env, rows, kind):
    check_deepfm(env, 10, rows, kind, seed=43)


def test_deepfm_33_domains_on_four_rows(env):
    check_deepfm(env, 33, 4, "mixed", seed=44)
