"""CPU restatement of the Star FAMILY (tests only): model_zoo/Star/star.py:70-96 with norm none / pn / bn, dense dense / star,
the auxiliary network and any hidden_dim -- oracle/star.py generalised, numpy fp32 with its rounding points.

`oracle/` is frozen, so this reference lives beside the tests.  For pn + star without the auxiliary network at three layers
every intermediate is computed by the statements of oracle/star.py (tests/test_star_forms_ref.py holds the two bit-equal).
PARITY UNPINNED like the oracle itself: TF 1.12 cannot be installed.  What is added to oracle/star.py's statement:
  * BatchNormalization (Keras defaults on a 2-d input, non-fused): the same nn.moments / nn.batch_normalization sequence
    with ONE gamma / beta pair; the moving pair is ONE for all domains, updated by Keras' `_assign_moving_average` of TF 1.12
    WITHOUT zero-debias: moving -= (moving - value) * float32(1.0 - 0.99).
  * AuxiliaryNet (auxiliary_net.py:100): a = relu(xn . kernel_specific[d] + bias_specific[d]) on the NORMALISED input
    (star.py:76-82), top = h_n + a (star.py:92-93).
  * Dense layers in StarFCN's place: plain kernels W_l, b_l.
`star_forward64` is the float64 torch FORWARD of the same family for autograd (as oracle/torch_ref.star_forward is for the
built form).  `FakeStarFormsEngine` is the CPU stand-in for GraphEngine("star", ...) in the host tests.
"""
import numpy as np

from oracle import star as ostar
from oracle import tower as T

F32 = np.float32
BN_DECAY = F32(1.0 - 0.99)      # Keras: decay = 1.0 - momentum as a Python float, cast to the variable's dtype


def param_names(emb_trainable, norm="pn", dense="star", auxiliary_dim=0, n_layers=3):
    emb = ("user_emb", "item_emb") if emb_trainable else ()
    k, b = ("Ws", "bs") if dense == "star" else ("W", "b")
    meta = emb + ("domain_emb",) + tuple("%s%d" % (k, l) for l in range(n_layers)) + tuple("%s%d" % (b, l) for l in range(n_layers))
    rest = ()
    if norm == "pn":
        rest += ("pn_gamma_shared", "pn_beta_shared", "pn_gamma_spec", "pn_beta_spec")
    elif norm == "bn":
        rest += ("bn_gamma", "bn_beta")
    if dense == "star":
        rest += tuple("Wd%d" % l for l in range(n_layers)) + tuple("bd%d" % l for l in range(n_layers))
    rest += ("wo", "gb")
    if auxiliary_dim:
        rest += ("aux_W", "aux_b")
    return meta, rest


def init_params(rs, n_user, n_item, n_domain, hidden=(256, 128, 64), norm="pn", dense="star", auxiliary_dim=0, emb_dim=128):
    p = {}
    p["user_emb"] = rs.uniform(-0.05, 0.05, (n_user, emb_dim)).astype(F32)
    p["item_emb"] = rs.uniform(-0.05, 0.05, (n_item, emb_dim)).astype(F32)
    p["domain_emb"] = rs.uniform(-0.05, 0.05, (n_domain, emb_dim)).astype(F32)
    dims = (3 * emb_dim,) + tuple(hidden)
    if norm == "pn":
        p["pn_gamma_shared"] = np.ones(dims[0], F32)
        p["pn_beta_shared"] = np.zeros(dims[0], F32)
        p["pn_gamma_spec"] = np.ones((n_domain, dims[0]), F32)
        p["pn_beta_spec"] = np.zeros((n_domain, dims[0]), F32)
    elif norm == "bn":
        p["bn_gamma"] = np.ones(dims[0], F32)
        p["bn_beta"] = np.zeros(dims[0], F32)
    for l in range(len(hidden)):
        if dense == "star":
            p["Ws%d" % l] = ostar.glorot_uniform(rs, (dims[l], dims[l + 1]), dims[l], dims[l + 1])
            p["Wd%d" % l] = ostar.glorot_uniform(rs, (n_domain, dims[l], dims[l + 1]), dims[l], dims[l + 1])
            p["bs%d" % l] = np.zeros(dims[l + 1], F32)
            p["bd%d" % l] = np.zeros((n_domain, dims[l + 1]), F32)
        else:
            p["W%d" % l] = ostar.glorot_uniform(rs, (dims[l], dims[l + 1]), dims[l], dims[l + 1])
            p["b%d" % l] = np.zeros(dims[l + 1], F32)
    p["wo"] = ostar.glorot_uniform(rs, (dims[-1], 1), dims[-1], 1)
    p["gb"] = np.zeros(1, F32)
    if auxiliary_dim:
        p["aux_W"] = ostar.glorot_uniform(rs, (n_domain, dims[0], auxiliary_dim), dims[0], auxiliary_dim)
        p["aux_b"] = np.zeros((n_domain, auxiliary_dim), F32)
    return p


def init_state(norm, n_domain, dim=384):
    if norm == "pn":
        return ostar.init_state(n_domain, dim)
    if norm == "bn":
        return {"mov_mean": np.zeros(dim, F32), "mov_var": np.ones(dim, F32)}
    return {}


def n_layers_of(params):
    n = 0
    while ("Ws%d" % n) in params or ("W%d" % n) in params:
        n += 1
    return n


def effective(params, d, norm, dense):
    n = n_layers_of(params)
    if norm == "pn":
        gamma = (params["pn_gamma_shared"] * params["pn_gamma_spec"][d]).astype(F32)
        beta = (params["pn_beta_shared"] + params["pn_beta_spec"][d]).astype(F32)
    elif norm == "bn":
        gamma, beta = params["bn_gamma"], params["bn_beta"]
    else:
        gamma = beta = None
    if dense == "star":
        K = [(params["Ws%d" % l] * params["Wd%d" % l][d]).astype(F32) for l in range(n)]
        b = [(params["bs%d" % l] + params["bd%d" % l][d]).astype(F32) for l in range(n)]
    else:
        K = [params["W%d" % l] for l in range(n)]
        b = [params["b%d" % l] for l in range(n)]
    return gamma, beta, K, b


def forward(params, state, uid, pid, dom, training, norm="pn", dense="star", auxiliary_dim=0):
    d = int(dom[0])
    x = T.gather(params, uid, pid, dom)
    gamma, beta, K, b = effective(params, d, norm, dense)
    c = dict(d=d, x=x, K=K)
    if norm == "none":
        xn = x
    else:
        if training:
            mean, var = ostar.batch_moments(x)
        elif norm == "pn":
            mean, var = state["mov_mean"][d], state["mov_var"][d]
        else:
            mean, var = state["mov_mean"], state["mov_var"]
        inv = (F32(1) / np.sqrt(var + ostar.PN_EPS, dtype=F32)).astype(F32)
        scale = (inv * gamma).astype(F32)
        xn = (x * scale + (beta - mean * scale).astype(F32)).astype(F32)
        c.update(mean=mean, var=var, inv=inv, gamma=gamma)
    hs = [xn]
    h = xn
    for l in range(len(K)):
        h = np.maximum((h @ K[l] + b[l]).astype(F32), F32(0))
        hs.append(h)
    top = h
    if auxiliary_dim:
        a = np.maximum((xn @ params["aux_W"][d] + params["aux_b"][d]).astype(F32), F32(0))
        top = (h + a).astype(F32)
        c["a"] = a
    logit = (top @ params["wo"]).astype(F32)[:, 0] + params["gb"][0]
    c.update(hs=hs, top=top)
    return T.sigmoid(logit), c


def update_moving(state, norm, d, mean, var):
    if norm == "pn":
        ostar.update_moving(state, d, mean, var)
    elif norm == "bn":
        for key, value in (("mov_mean", mean), ("mov_var", var)):
            state[key] -= ((state[key] - value).astype(F32) * BN_DECAY).astype(F32)


def loss_and_grads(params, state, uid, pid, dom, label, emb_trainable, norm="pn", dense="star", auxiliary_dim=0):
    B = uid.shape[0]
    p, c = forward(params, state, uid, pid, dom, True, norm, dense, auxiliary_dim)
    d, hs, K = c["d"], c["hs"], c["K"]
    n = len(K)
    y = label.astype(F32)
    loss = F32(np.mean(T.bce_per_row(p, y), dtype=np.float64))
    inside = ((p >= T.EPS_CLIP) & (p <= F32(1) - T.EPS_CLIP)).astype(F32)
    dlogit = ((p - y) * inside / F32(B)).astype(F32)
    big = [t for t in ("user_emb", "item_emb") if emb_trainable and T.bigtable.use_rows(params[t])]
    names = sum(param_names(emb_trainable, norm, dense, auxiliary_dim, n), ())
    g = {t: np.zeros_like(params[t]) for t in names if t not in big}
    g["wo"] = (c["top"].T @ dlogit[:, None]).astype(F32)
    g["gb"] = np.array([np.sum(dlogit, dtype=np.float64)], F32)
    dtop = (dlogit[:, None] * params["wo"][:, 0][None, :]).astype(F32)
    dh = dtop
    for l in range(n - 1, -1, -1):
        dz = (dh * (hs[l + 1] > 0)).astype(F32)
        dK = (hs[l].T @ dz).astype(F32)
        db = np.sum(dz, axis=0, dtype=np.float64).astype(F32)
        if dense == "star":
            g["Ws%d" % l] = (dK * params["Wd%d" % l][d]).astype(F32)
            g["Wd%d" % l][d] = (dK * params["Ws%d" % l]).astype(F32)
            g["bs%d" % l] = db
            g["bd%d" % l][d] = db
        else:
            g["W%d" % l] = dK
            g["b%d" % l] = db
        dh = (dz @ K[l].T).astype(F32)
    dxn = dh
    if auxiliary_dim:
        dza = (dtop * (c["a"] > 0)).astype(F32)
        g["aux_W"][d] = (hs[0].T @ dza).astype(F32)
        g["aux_b"][d] = np.sum(dza, axis=0, dtype=np.float64).astype(F32)
        dxn = (dxn + (dza @ params["aux_W"][d].T).astype(F32)).astype(F32)
    if norm == "none":
        dx = dxn
    else:
        xhat = ((c["x"] - c["mean"]) * c["inv"]).astype(F32)
        s1 = np.sum(dxn, axis=0, dtype=np.float64).astype(F32)
        s2 = np.sum((dxn * xhat).astype(F32), axis=0, dtype=np.float64).astype(F32)
        if norm == "pn":
            g["pn_beta_shared"] = s1
            g["pn_beta_spec"][d] = s1
            g["pn_gamma_shared"] = (s2 * params["pn_gamma_spec"][d]).astype(F32)
            g["pn_gamma_spec"][d] = (s2 * params["pn_gamma_shared"]).astype(F32)
        else:
            g["bn_beta"] = s1
            g["bn_gamma"] = s2
        coef = (c["gamma"] * c["inv"]).astype(F32)
        dx = (coef * (dxn - (s1 / F32(B)).astype(F32) - (xhat * (s2 / F32(B)).astype(F32)).astype(F32))).astype(F32)
    E = params["domain_emb"].shape[1]
    for j in np.unique(dom):        # rows of each domain in batch order (a uniform batch: oracle/star.py's one sum)
        g["domain_emb"][j] = np.sum(dx[dom == j, 2 * E:], axis=0, dtype=np.float64).astype(F32)
    if emb_trainable:
        for name, ids, cols in (("user_emb", uid, slice(0, E)), ("item_emb", pid, slice(E, 2 * E))):
            if name in big:
                g[name] = T.bigtable.RowGrad(params[name], ids, dx[:, cols], 0.0)
                continue
            gt = np.zeros_like(params[name], dtype=np.float64)
            np.add.at(gt, ids, dx[:, cols].astype(np.float64))
            g[name] = gt.astype(F32)
    return loss, g, p, c


class StarForms(object):
    """stand-in for the compiled Keras Star model of any form: OracleStar's surface."""

    def __init__(self, params, norm="pn", dense="star", auxiliary_dim=0, emb_trainable=True, lr=1e-3):
        self.params = params
        self.norm, self.dense, self.auxiliary_dim = norm, dense, int(auxiliary_dim)
        self.emb_trainable = emb_trainable
        self.meta_names, self.rest_names = param_names(emb_trainable, norm, dense, auxiliary_dim, n_layers_of(params))
        self.names = self.meta_names + self.rest_names
        self.state = init_state(norm, params["domain_emb"].shape[0], 3 * params["domain_emb"].shape[1])
        self.opt = T.Optimizer(params, self.names)
        self.lr = lr
        self.use_sgd = False
        self.step = 0

    def form(self):
        return dict(norm=self.norm, dense=self.dense, auxiliary_dim=self.auxiliary_dim)

    def get_flat(self, meta_only=False):
        return T.flatten(self.params, self.meta_names if meta_only else self.names)

    def set_flat(self, vec, meta_only=False):
        T.unflatten(vec, self.params, self.meta_names if meta_only else self.names)

    def loss_and_grads(self, uid, pid, dom, label):
        return loss_and_grads(self.params, self.state, uid, pid, dom, label, self.emb_trainable, **self.form())

    def train_on_batch(self, uid, pid, dom, label):
        loss, g, _, c = self.loss_and_grads(uid, pid, dom, label)
        if self.norm != "none":
            update_moving(self.state, self.norm, c["d"], c["mean"], c["var"])
        if self.use_sgd:
            self.opt.sgd(self.params, g, self.lr)
        else:
            self.opt.adam(self.params, g, self.lr)
        self.step += 1
        return loss

    def accumulate_on_batch(self, acc, uid, pid, dom, label):
        """a meta pass' step (maml.py:196-229): the layer runs in training mode -- the moving statistics move --, the
        gradient is added to `acc` (a flat vector in `names` order), the weights stay."""
        loss, g, _, c = self.loss_and_grads(uid, pid, dom, label)
        if self.norm != "none":
            update_moving(self.state, self.norm, c["d"], c["mean"], c["var"])
        off = 0
        for n in self.names:
            cnt = self.params[n].size
            gn = g[n].dense() if hasattr(g[n], "dense") else g[n]
            acc[off:off + cnt] += np.asarray(gn, F32).ravel()
            off += cnt
        return loss

    def train_pass(self, data, perm, batch_size, max_steps=0, accumulate_into=None):
        n = perm.shape[0]
        n_step = -(-n // batch_size)
        if max_steps > 0:
            n_step = min(n_step, max_steps)
        out = []
        for s in range(n_step):
            idx = perm[s * batch_size:(s + 1) * batch_size]
            args = (data["uid"][idx], data["pid"][idx], data["domain"][idx], data["label"][idx])
            out.append(self.accumulate_on_batch(accumulate_into, *args) if accumulate_into is not None
                       else self.train_on_batch(*args))
        return out

    def evaluate(self, data, batch_size):
        n = data["uid"].shape[0]
        batch_losses = []
        preds = np.empty(n, F32)
        for s in range(0, n, batch_size):
            sl = slice(s, min(n, s + batch_size))
            p, _ = forward(self.params, self.state, data["uid"][sl], data["pid"][sl], data["domain"][sl], False, **self.form())
            preds[sl] = p
            batch_losses.append(F32(np.mean(T.bce_per_row(p, data["label"][sl].astype(F32)), dtype=np.float64)))
        return F32(np.mean(np.array(batch_losses, np.float64))), preds


# ---------------------------------------------------------------------------------------------- float64 autograd (forward only)
def star_forward64(P, uid, pid, dom, norm, dense, auxiliary_dim, n_layers):
    """torch forward of the family (training mode: batch statistics); returns (p, mean, var) -- mean / var None without a norm."""
    import torch
    d = int(dom[0])
    x = torch.cat([P["user_emb"][uid], P["item_emb"][pid], P["domain_emb"][dom]], dim=1)
    mean = var = None
    xn = x
    if norm != "none":
        mean = x.mean(dim=0)
        var = ((x - mean) ** 2).mean(dim=0)
        if norm == "pn":
            gamma = P["pn_gamma_shared"] * P["pn_gamma_spec"][d]
            beta = P["pn_beta_shared"] + P["pn_beta_spec"][d]
        else:
            gamma, beta = P["bn_gamma"], P["bn_beta"]
        xn = (x - mean) * torch.rsqrt(var + 1e-3) * gamma + beta
    h = xn
    for l in range(n_layers):
        if dense == "star":
            h = torch.relu(h @ (P["Ws%d" % l] * P["Wd%d" % l][d]) + P["bs%d" % l] + P["bd%d" % l][d])
        else:
            h = torch.relu(h @ P["W%d" % l] + P["b%d" % l])
    if auxiliary_dim:
        h = h + torch.relu(xn @ P["aux_W"][d] + P["aux_b"][d])
    logit = (h @ P["wo"])[:, 0] + P["gb"][0]
    return torch.sigmoid(logit), mean, var


def loss_and_grads64(params, names, uid, pid, dom, label, norm, dense, auxiliary_dim):
    """float64 autograd of the Keras BCE (1e-7 clip) mean over the batch; gradients of every tensor in `names`."""
    import torch
    P = {n: torch.tensor(np.asarray(params[n], np.float64), requires_grad=n in names) for n in params}
    ui, pi, di = (torch.from_numpy(np.asarray(a, np.int64)) for a in (uid, pid, dom))
    y = torch.from_numpy(np.asarray(label, np.float64))
    p, mean, var = star_forward64(P, ui, pi, di, norm, dense, auxiliary_dim, n_layers_of(params))
    from oracle import torch_ref as tref
    loss = tref.keras_bce(p, y).mean()
    grads = torch.autograd.grad(loss, [P[n] for n in names], allow_unused=True)
    g = {n: (gr.numpy() if gr is not None else np.zeros(params[n].shape)) for n, gr in zip(names, grads)}
    extra = {} if mean is None else {"mean": mean.detach().numpy(), "var": var.detach().numpy()}
    return float(loss.detach()), g, p.detach().numpy(), extra


# ---------------------------------------------------------------------------------------------- host tests' engine stand-in
def fake_star_graph(kind, n_user, n_item, n_domain, batch_size, expert_hidden, tower_hidden=(), dropout=0.0,
                    emb_trainable=False, emb_dim=128, norm="pn", dense="star", auxiliary_dim=0, **kw):
    """factory.star_graph of the host tests: GraphEngine("star", ...)'s call signature on StarForms."""
    from fake_engine import FakeEngine
    from mamdr_amd.graph_engine import star_keras_names

    class FakeStarFormsEngine(FakeEngine):
        def __init__(self):
            import torch
            assert kind == "star" and emb_dim == 128
            self.kind, self.norm, self.dense, self.auxiliary_dim = kind, norm, dense, int(auxiliary_dim)
            self.created_with = dict(kind=kind, expert_hidden=tuple(expert_hidden), dropout=dropout, emb_trainable=emb_trainable,
                                     norm=norm, dense=dense, auxiliary_dim=int(auxiliary_dim))
            self.n_user, self.n_item, self.n_domain = n_user, n_item, n_domain
            self.batch_size = batch_size
            self.device = torch.device("cpu")
            self.dropout_seed = kw.get("dropout_seed", 1024)
            params = init_params(np.random.RandomState(0), n_user, n_item, n_domain, tuple(expert_hidden), norm, dense,
                                 auxiliary_dim)
            self.oracle = StarForms(params, norm, dense, auxiliary_dim, emb_trainable=emb_trainable)
            self.segments, off = {}, 0
            for name in self.oracle.names:
                self.segments[name] = (off, params[name].size)
                off += params[name].size
            self.n_params = self.n_meta = off
            self.aux = None
            st = self.oracle.state
            if norm != "none":          # aux aliases the reference's state, in the HIP engine's layout
                keys = ("mov_mean", "mov_var", "biased_mean", "biased_var") if norm == "pn" else ("mov_mean", "mov_var")
                D, X = (n_domain, 384) if norm == "pn" else (1, 384)
                steps = D if norm == "pn" else 0
                self._aux_np = np.zeros((len(keys) * D * X + steps + 3) // 4 * 4, F32)
                for k, key in enumerate(keys):
                    view = self._aux_np[k * D * X:(k + 1) * D * X].reshape(st[key].shape)
                    view[...] = st[key]
                    st[key] = view
                if steps:
                    view = self._aux_np[4 * D * X:4 * D * X + D]
                    view[...] = st["steps"]
                    st["steps"] = view
                self.aux = torch.from_numpy(self._aux_np)
            self.data, self.calls = {}, []
            self._ema = None

        def keras_name(self, segment):
            return star_keras_names(self.segments, self.dense).get(segment, segment)

    return FakeStarFormsEngine()
