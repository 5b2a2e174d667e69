"""BaseModel -- host-side mirror of the reference's model_zoo/base_model.py.

Keeps the control flow and the files a user of the reference relies on:
checkpoint / result paths (base_model.py:23-28), `val_and_test` (base_model.py:111-144),
the weighted AUC print (base_model.py:157-175), the patience counter that treats
`metric <= best` as no improvement (base_model.py:202-224), per-domain finetuning with
Keras EarlyStopping(val_AUC, min_delta=1e-4) + best-only checkpoint semantics
(base_model.py:41-109) and `save_result` (base_model.py:183-200).  Numerics go through
`self.model`, a `TowerEngine` (the compiled Keras model's stand-in).  Weights are saved
as .npz (h5py is not available): the flat trainable vector plus its segment table.
"""
import json
import os
import os.path as osp
import time

import numpy as np

from .. import meta, parallel
from .. import plan as mplan
from ..reports import EVAL_REPORTS, requested


class BaseModel(object):
    def __init__(self, dataset, config, engine_factory=None):
        self.n_uid = dataset.n_uid
        self.n_pid = dataset.n_pid
        self.n_domain = dataset.n_domain
        self.dataset = dataset
        self.config = config
        self.model_config = config["model"]
        self.train_config = config["train"]
        self.engine_factory = engine_factory
        stamp = time.strftime("%a-%b-%d-%H-%M-%S", time.localtime())
        self.checkpoint_path = osp.join(self.train_config["checkpoint_path"], self.model_config["name"],
                                        dataset.conf["name"], dataset.conf["domain_split_path"], stamp,
                                        "model_parameters.npz")
        self.result_path = osp.join(self.train_config["result_save_path"], self.model_config["name"],
                                    dataset.conf["name"], dataset.conf["domain_split_path"])
        self.learning_rate = self.train_config["learning_rate"]
        self.batch_size = dataset.batch_size
        sizes = {d: v["n_data"] for d, v in dataset.train_dataset.items()}
        self.shuffler = mplan.PassShuffler(sizes, dataset.shuffle_buffer_size, dataset.seed,
                                           shuffle=getattr(dataset, "shuffle_train", True))
        self.reports = {e.name: {} for e in EVAL_REPORTS}        # {name: {(mode, domain): the latest evaluation's report}}
        self.gauc_reports, self.exact_reports, self.ci_reports = (self.reports[n] for n in ("gauc", "exact", "ci"))
        self.model = self.build_model()
        self._build_early_stop()

    def build_model(self):
        raise NotImplementedError("You must implement build model")

    def train(self):
        raise NotImplementedError

    # ------------------------------------------------------------------ build_model's shared steps
    def pretrained_tables(self):
        """(user, item) tables of the dataset when train.load_pretrain_emb is set, else (None, None)."""
        if not self.train_config["load_pretrain_emb"]:
            return None, None
        user, item = self.dataset.user_emb, self.dataset.item_emb
        if user is None:
            raise ValueError("load_pretrain_emb is set but the dataset has no pretrained tables")
        for what, table in (("user", user), ("item", item)):
            if table is not None and table.shape[1] != self.model_config["user_dim"]:
                raise ValueError("the pretrained %s table is %d wide, model.user_dim says %d (synthetic data: "
                                 "dataset.synthetic_emb_dim)" % (what, table.shape[1], self.model_config["user_dim"]))
        return user, item

    def construct_engine(self, r):
        """the engine of a deepctr.Route: the HIP engines -- looked up in their modules now --, or the injected factory:
        itself, or the attribute of it the route names."""
        tc = self.train_config
        # deepctr.py:104-116: `trainable=emb_trainable` reaches SparseFeat only on the pretrained branch; without
        # pretrained tables the column is built with deepctr's default (trainable) WHATEVER emb_trainable says
        self.tables_trainable = bool(tc["emb_trainable"]) or not bool(tc["load_pretrain_emb"])
        factory = self.engine_factory
        if factory is None:
            from .. import engine, graph_engine
            factory = graph_engine.GraphEngine if r.engine == "graph" else engine.TowerEngine
        elif r.offer:
            factory = getattr(factory, r.offer)
        eng = factory(*r.args, self.n_uid, self.n_pid, self.n_domain, self.batch_size, emb_trainable=self.tables_trainable,
                      **r.kwargs)
        if hasattr(eng, "enable_retrieval"):        # GraphEngine: its mlp / wdl / deepfm kinds serve recommend ... once asked to
            eng.enable_retrieval()
        return eng

    def bind_engine(self, eng, tensors, where):
        """frozen tables, the three splits' columns, the initial weights, the compiled optimiser."""
        tc = self.train_config
        if not self.tables_trainable:
            eng.bind_table("user_emb", tensors["user_emb"])
            eng.bind_table("item_emb", tensors["item_emb"])
        for split, store in (("train", self.dataset.train_dataset), ("val", self.dataset.val_dataset),
                             ("test", self.dataset.test_dataset)):
            for d, v in store.items():
                c = v["data"]
                eng.bind_domain_data(d, split, c["uid"], c["pid"], c["domain"], c["label"])
        eng.set_weights(eng.pack(tensors))
        self.optimizer = tc["optimizer"]
        eng.compile(self.optimizer)      # "adam" -> tf.train.AdamOptimizer(learning_rate); a Keras name otherwise (deepctr.py:54-57)
        if tc["loss"] != "binary_crossentropy":
            raise NotImplementedError("loss '%s': only binary_crossentropy is %s" % (tc["loss"], where))
        return eng

    # ------------------------------------------------------------------ step / eval primitives
    def fit_domain(self, idx, max_steps=0, optimizer="adam", lr=None, trace=None, phase="fit"):
        """model.fit(iter, steps_per_epoch=n_step) / n_step x train_on_batch on one domain."""
        return meta.run_pass(self.model, idx, self.shuffler, self.batch_size,
                             self.learning_rate if lr is None else lr, trace if trace is not None else [],
                             phase, max_steps, optimizer)

    def evaluate_domain(self, idx, mode):
        """model.evaluate(d['data'], steps=d['n_step']) -> (loss, auc).  It also yields every report of reports.EVAL_REPORTS
        whose train-config key is set (no key of the reference's configs), of whatever weights the caller has installed, kept
        per (mode, domain) for _summarise / save_result; every decision stays on the 500-threshold AUC."""
        wanted = requested(self.train_config)
        out = self.model.evaluate(idx, mode, **{e.keyword: req for e, req in wanted})   # (an engine sees a keyword only when its key is set)
        for (e, _), report in zip(wanted, out[2:]):           # the tuple's tail, in table order
            self.reports[e.name][(mode, idx)] = report
        return out[:2]

    # ------------------------------------------------------------------ retrieval (no reference counterpart)
    def _retrieval_problem(self, domain, users, exclude_seen):
        """what `recommend`, `rank_eval` and `sampled_eval` ask of `domain` -> (catalogue: the distinct pids of its three splits; users:
        the given ones, by default the distinct uids of its test split; exclude: per user the items it has in the domain's
        train or val split, None when exclude_seen is off)."""
        cols = [s[domain]["data"] for s in (self.dataset.train_dataset, self.dataset.val_dataset, self.dataset.test_dataset)
                if domain in s]
        catalogue = np.unique(np.concatenate([np.asarray(c["pid"], np.int64) for c in cols]))
        if users is None:
            users = np.unique(np.asarray(self.dataset.test_dataset[domain]["data"]["uid"], np.int64))
        users = np.asarray(users, np.int64).ravel()
        exclude = None
        if exclude_seen:
            seen = {}
            for store in (self.dataset.train_dataset, self.dataset.val_dataset):
                if domain in store:
                    c = store[domain]["data"]
                    for u, p in zip(np.asarray(c["uid"]).tolist(), np.asarray(c["pid"]).tolist()):
                        seen.setdefault(u, []).append(p)
            exclude = [seen.get(int(u), ()) for u in users]
        return catalogue, users, exclude

    def recommend(self, domain, k, users=None, exclude_seen=True):
        """top-k items of `domain`'s catalogue -- the distinct pids of its three splits -- for `users` (default: the distinct
        uids of its test split) from the live weights.  exclude_seen: a user never gets an item it has in the domain's train
        or val split.  -> {"users" [Q], "ids" [Q, k] (-1 behind a short list), "scores" [Q, k], "catalogue": its size}."""
        catalogue, users, exclude = self._retrieval_problem(domain, users, exclude_seen)
        # one domain per call: the engine's single-domain retrieval where it has one (the only one the Star tower has)
        single = getattr(self.model, "recommend_domain", None)
        if single is not None:
            ids, scores = single(users, int(domain), k, candidates=catalogue, exclude=exclude)[:2]
        else:
            ids, scores = self.model.recommend(users, np.full(users.shape, domain, np.int64), k, candidates=catalogue,
                                               exclude=exclude)[:2]
        return {"users": users, "ids": ids, "scores": scores, "catalogue": int(catalogue.shape[0])}

    def rank_eval(self, domain, users=None, exclude_seen=True):
        """the exact rank, in `domain`'s whole catalogue, of every held-out positive -- the label-1 items of its test split --
        of `users` (default: the distinct uids of its test split) from the live weights (the engine's rank_domain:
        mamdr_rank_domain).  exclude_seen: the items a user has in the domain's train or val split are not candidates.
        -> the engine's dict ("offsets", "ids", "ranks", "listed", "live") plus "users" [Q], "catalogue" (the candidate ids)
        and "n_positives" [Q] (the distinct positives of each user)."""
        from .. import recommend as rec
        catalogue, users, exclude = self._retrieval_problem(domain, users, exclude_seen)
        positives = rec.split_positives(self.dataset, domain, users)
        res = dict(self.model.rank_domain(users, int(domain), positives, candidates=catalogue, exclude=exclude))
        res.update(users=users, catalogue=catalogue, n_positives=np.diff(res["offsets"]).astype(np.int64))
        return res

    def rerank(self, domain, users, slates):
        """every user's own candidate slate -- `slates`: one array of distinct item ids per user, in the caller's order --
        scored and ordered in `domain` from the live weights (the engine's rank_slates: mamdr_rank_slates) -> the engine's
        dict ("offsets", "ids", "scores", "pos") plus "users" [Q]."""
        users = np.asarray(users, np.int64).ravel()
        res = dict(self.model.rank_slates(users, int(domain), slates))
        res["users"] = users
        return res

    def sampled_eval(self, domain, n_neg, seed=0, users=None, exclude_seen=True):
        """the sampled-negatives protocol on `domain`: one slate per distinct (user, positive) pair of its test split (label
        1; `users`: default the distinct uids of that split) -- entry 0 the positive, behind it `n_neg` negatives drawn
        uniformly without replacement (recommend.sample_negatives, `seed`) from the domain's catalogue (_retrieval_problem's)
        without the user's train / val items (exclude_seen) and without ANY of the user's test positives.  A user with fewer
        free items than n_neg gets all of them: such slates are evaluated and counted in "n_short".
        -> `rerank`'s dict ("users" [S]: the user of each slate) plus "positives" [S], "rank" [S] (pos of entry 0: the
        negatives that order before the positive), "slate_len" [S] and "n_short"."""
        from .. import recommend as rec
        catalogue, users, exclude = self._retrieval_problem(domain, users, exclude_seen)
        positives = [np.unique(p) for p in rec.split_positives(self.dataset, domain, users)]
        n_pos = np.asarray([p.size for p in positives], np.int64)
        forbid = [np.concatenate([np.asarray(exclude[q] if exclude is not None else (), np.int64).ravel(), p])
                  for q, p in enumerate(positives)]
        f_len = np.asarray([f.size for f in forbid], np.int64)
        by_slate = np.repeat(np.arange(users.size), n_pos)          # slate -> index of its user
        slate_users = users[by_slate]
        slate_pos = np.concatenate(positives + [np.zeros(0, np.int64)])
        # the users' forbidden lists, once per slate of the user
        f_start = np.concatenate([[0], np.cumsum(f_len)])[:-1]
        f_off = np.concatenate([[0], np.cumsum(f_len[by_slate])]).astype(np.int64)
        f_all = np.concatenate(forbid + [np.zeros(0, np.int64)])
        f_ids = f_all[np.repeat(f_start[by_slate] - f_off[:-1], f_len[by_slate]) + np.arange(f_off[-1])]
        n_off, n_ids = rec.sample_negatives(catalogue, f_off, f_ids, n_neg, seed)
        n_slate = slate_pos.size
        off = n_off + np.arange(n_slate + 1)
        ids = np.empty(int(off[-1]), np.int64)
        is_pos = np.zeros(ids.size, bool)
        is_pos[off[:-1]] = True
        ids[is_pos], ids[~is_pos] = slate_pos, n_ids
        res = self.rerank(domain, slate_users, np.split(ids, off[1:-1]) if n_slate else [])
        slate_len = np.diff(off)
        res.update(positives=slate_pos, rank=res["pos"][off[:-1]], slate_len=slate_len,
                   n_short=int((slate_len < int(n_neg) + 1).sum()))
        return res

    # ------------------------------------------------------------------ what the lists are made of (no reference counterpart)
    def list_eval(self, domain, k):
        """what list_metrics.summarise needs of `domain`, from the live weights: the lists of `recommend(domain, k)` and, on
        the device, their exposure counts and the train split's label-1 popularity counts (the engine's id_counts:
        mamdr_id_counts, over the whole item range) and the lists' pairwise similarity on the engine's item_rows() -- the
        item table of the same weights -- (list_similarity: mamdr_list_similarity).  -> {"users" [Q], "ids" [Q, k],
        "catalogue" (the candidate ids), "exposure" / "popularity" [n_item] int64, "sim_sum" [Q] float64, "pairs" [Q]
        int32}.  It reads state only."""
        import torch
        from .. import list_metrics
        k = list_metrics.check_k(k)
        eng = self.model
        r = self.recommend(domain, k)
        catalogue = self._retrieval_problem(domain, r["users"], False)[0]
        ids = torch.from_numpy(np.ascontiguousarray(r["ids"], np.int32)).to(eng.device)
        n_item = int(eng.n_item)
        exposure = eng.id_counts(ids, n_item)
        popularity = None
        if domain in self.dataset.train_dataset:
            cols = eng.data[(domain, "train")]
            popularity = eng.id_counts(cols["pid"], n_item, cols["label"])
        sim_sum, pairs = eng.list_similarity(ids, eng.item_rows()) if ids.shape[0] else (np.zeros(0), np.zeros(0, np.int32))
        def counts(t):          # (a device tensor holds the uint32 counts as int32: reinterpret, do not convert)
            a = list_metrics.to_host(t)
            return (a.view(np.uint32) if a.dtype == np.int32 else a).astype(np.int64)
        return {"users": r["users"], "ids": r["ids"], "catalogue": catalogue, "exposure": counts(exposure),
                "popularity": counts(popularity) if popularity is not None else np.zeros(n_item, np.int64),
                "sim_sum": list_metrics.to_host(sim_sum).astype(np.float64), "pairs": list_metrics.to_host(pairs).astype(np.int32)}

    # ------------------------------------------------------------------ diversified re-ranking (no reference counterpart)
    def diversify(self, domain, k, pool, lam, relevance="minmax"):
        """`domain`'s top-`pool` lists of `recommend(domain, pool)` re-ranked to k items each by greedy Maximal Marginal
        Relevance on the engine's item_rows() (list_diversify: mamdr_list_diversify) from the live weights.  relevance:
        "minmax" -- each list's scores scaled to [0, 1] on the device, list_metrics.minmax_relevance's fp32 formula -- or
        "score" -- the scores as they are.  -> {"users" [Q], "ids" [Q, k] (-1 behind a short list), "scores" [Q, k] (the
        picked items' scores), "pos" [Q, k] (their positions in the pool), "values" [Q, k] (what each pick won with),
        "base_ids" [Q, k] (the pool's first k: `recommend(domain, k)`'s lists), "pool_ids" [Q, pool], "catalogue": its
        size}.  With lam = 1 and "score" the picks are the base lists (as long as no two of a list's scores that the
        tower tells apart round to the same fp32 probability).  It reads state only."""
        import torch
        from .. import list_metrics
        k, pool = list_metrics.check_pool(k, pool)
        lam = list_metrics.check_lambda(lam)
        if relevance not in ("minmax", "score"):
            raise ValueError("diversify: relevance %r is neither 'minmax' nor 'score'" % (relevance,))
        eng = self.model
        r = self.recommend(domain, pool)
        pool_ids = np.ascontiguousarray(r["ids"])
        ids = torch.from_numpy(pool_ids.astype(np.int32)).to(eng.device)
        scores = torch.from_numpy(np.ascontiguousarray(r["scores"], np.float32)).to(eng.device)
        rows = eng.item_rows()
        rel = scores
        if relevance == "minmax":
            valid = (ids >= 0) & (ids < int(rows.shape[0]))
            inf = torch.full_like(scores, float("inf"))
            lo = torch.where(valid, scores, inf).amin(dim=1, keepdim=True)
            hi = torch.where(valid, scores, -inf).amax(dim=1, keepdim=True)
            rel = torch.where(valid & (hi > lo), (scores - lo) / (hi - lo), torch.zeros_like(scores))
        if ids.shape[0]:
            pos, values = eng.list_diversify(ids, rel.contiguous(), rows, k, lam, want_values=True)
        else:
            pos, values = np.zeros((0, k), np.int32), np.zeros((0, k), np.float32)
        pos = torch.as_tensor(pos).to(torch.int64)
        at = pos.clamp(min=0)
        picked_ids = torch.where(pos >= 0, ids.gather(1, at), torch.full_like(ids[:, :k], -1))
        picked_scores = torch.where(pos >= 0, scores.gather(1, at), torch.zeros_like(scores[:, :k]))
        return {"users": r["users"], "ids": list_metrics.to_host(picked_ids).astype(pool_ids.dtype),
                "scores": list_metrics.to_host(picked_scores), "pos": list_metrics.to_host(pos).astype(np.int32),
                "values": np.asarray(list_metrics.to_host(values), np.float32), "base_ids": pool_ids[:, :k].copy(),
                "pool_ids": pool_ids, "catalogue": r["catalogue"]}

    def diversify_eval(self, domain, k, pool, lam, relevance="minmax"):
        """what list_metrics.diversify_report needs of `domain`: `diversify`'s dict plus, as list_eval gives them and from
        the same weights, "catalogue_ids", "popularity" [n_item] and, for the re-ranked lists, "exposure" [n_item] /
        "sim_sum" [Q] / "pairs" [Q], and for the base lists "base_exposure" / "base_sim_sum" / "base_pairs"."""
        import torch
        from .. import list_metrics
        eng = self.model
        res = self.diversify(domain, k, pool, lam, relevance)
        n_item = int(eng.n_item)
        def counts(t):          # (a device tensor holds the uint32 counts as int32: reinterpret, do not convert)
            a = list_metrics.to_host(t)
            return (a.view(np.uint32) if a.dtype == np.int32 else a).astype(np.int64)
        res["catalogue_ids"] = self._retrieval_problem(domain, res["users"], False)[0]
        res["popularity"] = np.zeros(n_item, np.int64)
        if domain in self.dataset.train_dataset:
            cols = eng.data[(domain, "train")]
            res["popularity"] = counts(eng.id_counts(cols["pid"], n_item, cols["label"]))
        rows = eng.item_rows()
        for pre, lists in (("base_", res["base_ids"]), ("", res["ids"])):
            ids = torch.from_numpy(np.ascontiguousarray(lists, np.int32)).to(eng.device)
            res[pre + "exposure"] = counts(eng.id_counts(ids, n_item))
            sim_sum, pairs = eng.list_similarity(ids, rows) if ids.shape[0] else (np.zeros(0), np.zeros(0, np.int32))
            res[pre + "sim_sum"] = list_metrics.to_host(sim_sum).astype(np.float64)
            res[pre + "pairs"] = list_metrics.to_host(pairs).astype(np.int32)
        return res

    # ------------------------------------------------------------------ similar items (no reference counterpart)
    def similar_items(self, domain, k, items=None, target_domain=None):
        """the k nearest neighbours by cosine, on the engine's item_rows() -- the item table of the live weights --, of
        `items` (default: `domain`'s catalogue, the distinct pids of its three splits) among the catalogue of
        `target_domain` (default: the same domain); an item is not its own neighbour (the engine's row_neighbours:
        mamdr_row_neighbours).  -> {"items" [Q], "ids" [Q, k] (-1 behind a short list), "sims" [Q, k] fp32, "catalogue"
        (the candidate ids)}.  It reads state only."""
        import torch
        from .. import list_metrics, neighbours
        k = neighbours.check_k(k)
        eng = self.model
        nobody = np.zeros(0, np.int64)
        catalogue = self._retrieval_problem(int(domain if target_domain is None else target_domain), nobody, False)[0]
        items = self._retrieval_problem(domain, nobody, False)[0] if items is None else np.asarray(items, np.int64).ravel()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(eng.device)
        if items.size and catalogue.size:
            ids, sims = eng.row_neighbours(eng.item_rows(), dev(items), k, candidates=dev(catalogue), exclude_self=True)
            ids, sims = list_metrics.to_host(ids), np.asarray(list_metrics.to_host(sims), np.float32)
        else:
            ids, sims = np.full((items.size, k), -1, np.int32), np.zeros((items.size, k), np.float32)
        return {"items": items, "ids": ids, "sims": sims, "catalogue": catalogue}

    # ------------------------------------------------------------------ isotonic recalibration (no reference counterpart)
    def isotonic_eval(self, domain, n_bins=20):
        """isotonic recalibration of `domain` from the live weights, on the device: the val and the test split are evaluated
        with their predictions kept there; the isotonic (PAV) fit of the val split is applied to the test split; the test
        split's Brier / log-loss sums and its ECE / PCOC over `n_bins` equal-mass bins (the existing exact metrics) are taken
        before and after; the test split's OWN fit gives the CORP decomposition of its Brier score.  -> isotonic.finish's
        report."""
        from .. import isotonic
        n_bins = isotonic.check_bins(n_bins)
        eng = self.model
        val_p, test_p = eng.predict_device(domain, "val"), eng.predict_device(domain, "test")
        val_y, test_y = eng.data[(domain, "val")]["label"], eng.data[(domain, "test")]["label"]
        val_fit, test_fit = eng.isotonic_fit(val_p, val_y), eng.isotonic_fit(test_p, test_y)
        fitted = eng.isotonic_apply(val_fit, test_p)
        return isotonic.finish(val_fit, test_fit, eng.score_sums(test_p, test_y), eng.score_sums(fitted, test_y),
                               eng.exact_metrics(test_p, test_y, n_bins), eng.exact_metrics(fitted, test_y, n_bins))

    # ------------------------------------------------------------------ domain conflict (no reference counterpart)
    def domain_conflict(self, n_batches=None):
        """conflict.measure at the live weights: one gradient per train domain over its first `n_batches` batches (None or 0:
        whole passes), their fp64 Gram matrices over the whole flat vector, the meta range and every tensor, the cosines
        and their summaries.  The engine's state is left as it was (engine.domain_gradients)."""
        from .. import conflict
        return conflict.measure(self.model, sorted(self.dataset.train_dataset), n_batches)

    # ------------------------------------------------------------------ finetune / separate training
    def separate_train_val_test(self, init_parms=True):
        """base_model.py:41-109.  init_parms=False is the finetune stage: plain SGD with
        `learning_rate` (base_model.py:69), restarted from the same weights for every domain.
        Under several processes (every rank holds the same weights) the domains are dealt round-robin."""
        weights = self.model.get_weights()
        if init_parms:
            self.model.optimizer_reset()
        rank, world = parallel.world()
        if world > 1:
            mine = [d for i, d in enumerate(self.dataset.train_dataset) if i % world == rank]
            _, _, dl, da = self._finetune_domains(lambda d: weights, "adam" if init_parms else "sgd", self.learning_rate,
                                                  domains=mine, summarise=False)
            dl, da = parallel.gather_domain_scalars({d: (dl[d], da[d]) for d in dl}, self.n_domain, self.model.device)
            return self._summarise("test", dl, da)
        return self._finetune_domains(lambda d: weights, "adam" if init_parms else "sgd", self.learning_rate)

    def _finetune_domains(self, start_weights, optimizer, lr, domains=None, summarise=True, per_domain_reset=False):
        domain_loss, domain_auc = {}, {}
        keep = self.model.get_weights()
        best = self.model.new_vector()
        self.finetune_log = {}        # {domain: epochs run, epoch of the kept checkpoint, val AUC per epoch}
        hook = getattr(self, "finetune_epoch_hook", None)       # tests: hook(domain, epoch, engine) after every epoch's pass
        for d in (self.dataset.train_dataset if domains is None else domains):
            self.model.set_weights(start_weights(d))
            if per_domain_reset:          # a freshly compiled optimiser per domain (deep_mtl_ctr.py:139-148)
                self.model.optimizer_reset()
            print("Train on domain: {}".format(d))
            # Keras EarlyStopping(monitor=val_AUC, mode=max, min_delta=1e-4) + ModelCheckpoint(best only)
            es_best, wait, ck_best = -np.inf, 0, -np.inf
            log = self.finetune_log[d] = {"epochs": 0, "best_epoch": -1, "val_auc": []}
            for epoch in range(self.train_config["epoch"]):
                self.fit_domain(d, optimizer=optimizer, lr=lr, phase="finetune")
                if hook is not None:
                    hook(d, epoch, self.model)
                _, val_auc = self.evaluate_domain(d, "val")
                log["epochs"] = epoch + 1
                log["val_auc"].append(float(val_auc))
                if val_auc > ck_best:
                    ck_best = val_auc
                    log["best_epoch"] = epoch
                    self.model.get_weights(out=best)
                if val_auc - 1e-4 > es_best:
                    es_best, wait = val_auc, 0
                else:
                    wait += 1
                    if wait >= self.train_config["patience"]:
                        break
            self.model.set_weights(best)
            p_loss, p_auc = self.evaluate_domain(d, "test")
            domain_loss[d], domain_auc[d] = float(p_loss), float(p_auc)
        self.model.set_weights(keep)
        if not summarise:
            return None, None, domain_loss, domain_auc
        return self._summarise("test", domain_loss, domain_auc)

    def val_and_test(self, mode):
        if mode not in ("val", "test"):
            raise ValueError("Mode can be either val or test, not: {}".format(mode))
        if mode == "test":
            self.load_model(self.checkpoint_path)      # best weights so far (base_model.py:121)
        domain_loss, domain_auc = {}, {}
        rank, world = parallel.world()
        for i, idx in enumerate(self.dataset.val_dataset if mode == "val" else self.dataset.test_dataset):
            if world > 1 and i % world != rank:        # every rank holds the same weights: deal the domains out
                continue
            p_loss, p_auc = self.evaluate_domain(idx, mode)
            domain_loss[idx], domain_auc[idx] = float(p_loss), float(p_auc)
        if world > 1:
            local = {d: (domain_loss[d], domain_auc[d]) for d in domain_loss}
            domain_loss, domain_auc = parallel.gather_domain_scalars(local, self.n_domain, self.model.device)
        return self._summarise(mode, domain_loss, domain_auc)

    def _summarise(self, mode, domain_loss, domain_auc):
        avg_loss = sum(domain_loss.values()) / len(domain_loss)
        avg_auc = sum(domain_auc.values()) / len(domain_auc)       # plain mean over domains
        print("Loss: ", domain_loss)
        self._format_print_domain_metric("AUC", domain_auc)
        print("Overall {} Loss: {}, AUC: {}, Weighted AUC: {}".format(mode, avg_loss, avg_auc,
                                                                     self._weighted_auc(mode, domain_auc)))
        for e, req in requested(self.train_config):
            e.print_summary(mode, self._reports_of(e, mode, domain_auc), req, self._format_print_domain_metric)
        return avg_loss, avg_auc, domain_loss, domain_auc

    def _reports_of(self, entry, mode, domains):
        store = self.reports[entry.name]          # -> {domain: the remembered report of `mode`}, in the order of `domains`
        return {d: store[(mode, d)] for d in domains if (mode, d) in store}

    def _format_print_domain_metric(self, name, domain_metric):
        print("{}: ".format(name))
        for key, value in domain_metric.items():
            print("{}: {}".format(key, value))

    def _weighted_auc(self, mode, domain_auc):
        info = self.dataset.dataset_info
        tag = "n_val" if "val" in mode else ("n_test" if "test" in mode else "n_train")
        total = sum(info[k][tag] for k in domain_auc)
        return sum(info[k][tag] * v for k, v in domain_auc.items()) / total

    # ------------------------------------------------------------------ persistence
    def save_model(self, path):
        aux = getattr(self.model, "aux", None)      # Star: PartitionedNorm moving statistics
        if path == self.checkpoint_path:            # the best-so-far checkpoint is also kept on the device
            self._best_in_memory = (self.model.get_weights().clone(), aux.clone() if aux is not None else None)
        if parallel.world()[0] != 0:                # one set of files per run
            return
        os.makedirs(osp.dirname(path) or ".", exist_ok=True)
        seg = self.model.segments
        np.savez(path, weights=self.model.get_weights().cpu().numpy(),
                 aux=aux.cpu().numpy() if aux is not None else np.zeros(0, np.float32),
                 segment_names=np.array(list(seg.keys())),
                 segment_offsets=np.array([v[0] for v in seg.values()], np.int64),
                 segment_counts=np.array([v[1] for v in seg.values()], np.int64))

    def load_model(self, path):
        import torch
        best = getattr(self, "_best_in_memory", None)
        if path == self.checkpoint_path and best is not None:
            self.model.set_weights(best[0])
            if best[1] is not None:
                self.model.aux.copy_(best[1])
            return
        with np.load(path) as z:
            w = z["weights"]
            aux = z["aux"] if "aux" in z.files else np.zeros(0, np.float32)
        if aux.size and getattr(self.model, "aux", None) is not None:
            self.model.aux.copy_(torch.from_numpy(aux).to(self.model.device))
        if w.shape[0] != self.model.n_params:
            raise ValueError("checkpoint has %d parameters, model has %d" % (w.shape[0], self.model.n_params))
        self.model.set_weights(torch.from_numpy(w).to(self.model.device))

    def save_result(self, avg_loss, avg_auc, domain_loss, domain_auc):
        folder = "loss_{:.3f}_auc_{:.3f}_{}".format(avg_loss, avg_auc, time.strftime("%a-%b-%d-%H-%M-%S",
                                                                                     time.localtime()))
        result_path = osp.join(self.result_path, folder)
        os.makedirs(result_path, exist_ok=True)
        with open(osp.join(result_path, "dataset_info.json"), "w") as f:
            json.dump(self.dataset.dataset_info, f)
        with open(osp.join(result_path, "config.json.example"), "w") as f:
            json.dump(self.config, f)
        with open(osp.join(result_path, "result.json"), "w") as f:
            result = {"avg_loss": avg_loss, "avg_auc": avg_auc, "domain_loss": domain_loss, "domain_auc": domain_auc}
            for e, req in requested(self.train_config):          # the test evaluations behind domain_auc
                e.save(result, result_path, self._reports_of(e, "test", domain_auc), req)
            json.dump(result, f)
        self.save_model(osp.join(result_path, "model_parameters.npz"))
        return result_path

    # ------------------------------------------------------------------ early stopping
    def _build_early_stop(self):
        self.patience = self.train_config["patience"]
        self.counter = 0
        self.best_metric = None
        self.early_stop = False

    def early_stop_step(self, metric):
        if self.best_metric is None:
            self.best_metric = metric
            self.save_model(self.checkpoint_path)
        elif metric <= self.best_metric:                    # ties count as "no improvement"
            self.counter += 1
            print("EarlyStopping counter: {} out of {}, Best AUC: {}".format(self.counter, self.patience,
                                                                           self.best_metric))
            if self.counter >= self.patience:
                self.early_stop = True
        else:
            self.save_model(self.checkpoint_path)
            self.best_metric = metric
            self.counter = 0
        return self.early_stop
