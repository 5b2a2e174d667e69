"""`run.py --config <json>` surface and the name registry (mirror of the reference's run.py).

Dispatch is by substring of config.model.name, in the reference's order (run.py:37-85):
  tower    'star' -> Star | any of mlp,wdl,nfm,autoint,ccpm,pnn,deepfm -> DeepCTR |
           shared_bottom,mmoe,ple -> DeepMTLCTR
  wrappers 'uncertainty_weight', 'pcgrad', then 'meta' + (domain_negotiation | mamdr |
           reptile | mldg | <else> MAML)
  modes    'separate' -> per-domain training; otherwise train() + val_and_test("test");
           'finetune' -> load best + separate_train_val_test(init_parms=False)
Every tower name of the reference's registries is built (run.py:37-47; deepctr.py:24-50: mlp wdl nfm autoint ccpm pnn
deepfm; deep_mtl_ctr.py:25-49: shared_bottom mmoe ple; star); Star in every form of star.py:70-96 -- norm none / pn / bn, dense dense / star, auxiliary_net); what is not (ple with more than one
level, uncertainty weighting on the multi-task towers) raises NotImplementedError naming why.
Not options of the reference's run.py: --lanes, --recommend K (top-K lists per domain, recommend.report), --gauc, --exact-metrics,
--auc-ci [B] with --auc-ci-unit and --auc-ci-seed (train.report_auc_ci: bootstrap intervals of the exact AUC, bootstrap.py), and
--rank-eval [KS] (train.rank_eval: the exact full-catalogue rank of every held-out positive, recommend.rank_report),
--sampled-eval [N] with --sampled-eval-ks KS (train.sampled_eval, train.sampled_eval_ks, train.sampled_eval_seed: every held-out
positive ranked among N sampled items the user never interacted with, recommend.sampled_report), and
--conflict [N] (train.conflict: the cosines between the domains' gradients on the same weights, conflict.report), and
--isotonic [B] with --isotonic-out FILE (train.isotonic: isotonic recalibration fitted on val, applied to test, and the CORP decomposition of the test Brier score, isotonic.report), and
--list-metrics [K] with --list-metrics-out FILE (train.list_metrics: what the top-K lists are made of -- coverage, Gini, entropy, novelty, tail share, personalisation and intra-list diversity per domain, list_metrics.report), and
--diversify [LAMBDA] with --diversify-pool N and --diversify-out FILE (train.diversify, train.diversify_pool, train.diversify_out: every test user's top-N pool re-ranked to K items by greedy Maximal Marginal Relevance on the device, with HitRate / NDCG and the list metrics of both the base and the re-ranked lists, list_metrics.diversify_report), and
--similar-items [K] with --similar-items-out FILE (train.similar_items, train.similar_items_out: every catalogue item's K exact cosine nearest neighbours on the item table, computed on the device, with the neighbour graph's hubness, orphan share and reciprocity per domain and the embedding-space affinity between the domains, neighbours.report), and
--baselines [SHRINK] with --baselines-out FILE and --baselines-max-items N (train.baselines, train.baselines_out, train.baselines_max_items; needs --rank-eval: MostPopular and ItemKNN -- cosine over the train split's co-occurrence counts with that shrinkage -- ranked on the device under the rank-eval protocol, printed beside the tower's own figures, with the overlap of their top-K lists with the tower's under --recommend K, baselines.report).
"""
import argparse
import json
import os

DEEP_CTR_LIST = ["mlp", "wdl", "nfm", "autoint", "ccpm", "pnn", "deepfm"]
MTL_DEEP_CTR_LIST = ["shared_bottom", "mmoe", "ple"]


def in_name_list(x, name_list):
    return any(n in x for n in name_list)


def build_model(config, dataset, engine_factory=None):
    from .model_zoo import MAML, MAMDR, MLDG, DeepCTR, DomainNegotiation, PCGrad, Reptile, Star, UncertaintyWeight
    name = config["model"]["name"]
    if "star" in name:
        model = Star(dataset, config, engine_factory)
    elif in_name_list(name, DEEP_CTR_LIST):
        model = DeepCTR(dataset, config, engine_factory)
    elif in_name_list(name, MTL_DEEP_CTR_LIST):
        from .model_zoo import DeepMTLCTR
        model = DeepMTLCTR(dataset, config, engine_factory)
    else:
        raise ValueError("model: {} not found".format(name))
    if "uncertainty_weight" in name:
        model = UncertaintyWeight(model)
    if "pcgrad" in name:
        model = PCGrad(model)
    if "meta" in name:
        if "domain_negotiation" in name:
            model = DomainNegotiation(model)
        elif "mamdr" in name:
            model = MAMDR(model)
        elif "reptile" in name:
            model = Reptile(model)
        elif "mldg" in name:
            model = MLDG(model)
        else:
            model = MAML(model)
    return model


def init_distributed():
    """one process per GPU when launched under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE in the
    environment): RCCL process group; MAMDR_SHARE_GPU=1 (testing on a 1-GPU box) keeps every rank on device 0
    over gloo.  Returns (rank, world_size)."""
    import os
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if ws <= 1:
        return 0, 1
    import torch
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        # an explicit timeout: a rank that hangs in the preflight's ring or in a collective is cut after
        # minutes, not after the backend's default of 10 - 30; MAMDR_COMM_TIMEOUT (seconds) overrides
        import datetime
        timeout = datetime.timedelta(seconds=float(os.environ.get("MAMDR_COMM_TIMEOUT", "300")))
        if os.environ.get("MAMDR_SHARE_GPU") == "1":
            if torch.cuda.is_available():
                torch.cuda.set_device(0)
            dist.init_process_group("gloo", timeout=timeout)
        else:
            # one process per GPU OF THIS NODE: LOCAL_WORLD_SIZE ranks share the node's devices (WORLD_SIZE counts the
            # ranks of every node)
            local_ws = int(os.environ.get("LOCAL_WORLD_SIZE", str(local + 1)))
            if torch.cuda.device_count() < max(local_ws, local + 1):
                raise RuntimeError("%d local ranks but %d visible GPUs (one process per GPU)" % (
                    max(local_ws, local + 1), torch.cuda.device_count()))
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", timeout=timeout)
        # first contact with the communicator: values of an all-reduce, a send / recv ring and a broadcast checked on
        # every rank; a failing ring switches the phi hand-over to broadcasts (parallel.preflight)
        from . import parallel
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        parallel.preflight(dev)
    return dist.get_rank(), dist.get_world_size()


def n_lanes(config):
    """train.lanes (not a key of the reference's configs; MAMDR_LANES overrides; default 1 = the reference's one
    sequential chain): the sharded epoch of SURVEY 8e run by that many LANES of this process on one GPU
    (parallel.LaneGroup) -- a lane run is the run of as many ranks, with the lanes' kernels overlapping on the device."""
    import os
    return max(1, int(os.environ.get("MAMDR_LANES") or config["train"].get("lanes", 1) or 1))


def main(config, engine_factory=None, on_model=None, recommend=None, recommend_out=None):
    """run.py:71-89.  on_model(model) (optional) sees the built, wrapped model before training starts (tests attach
    their recorders there).  recommend = K (not an option of the reference's run.py): once the pipeline has ended, rank 0 /
    lane 0 ranks every domain's catalogue for its test users with the weights the run finished with and writes the top K
    (recommend.report) to recommend_out, by default under train.result_save_path.  train.report_gauc, train.report_exact
    = B and train.report_auc_ci = B (run.py --gauc, --exact-metrics [B], --auc-ci [B]; no keys of the reference's configs):
    every evaluation also yields the reports of reports.EVAL_REPORTS -- the per-user grouped AUC (gauc.py); the exact AUC,
    average precision and calibration over B equal-mass bins (exact.py); B bootstrap replicates of the exact AUC by
    train.auc_ci_unit = "user" (default) or "row" under train.auc_ci_seed (default 0) (bootstrap.py).  train.rank_eval = [K,
    ...] (run.py --rank-eval; not a key of the reference's configs either): once the pipeline has ended, the exact rank of every
    test positive in its domain's whole catalogue, with MRR, mean percentile and HitRate / Recall / NDCG at those K
    (recommend.rank_report), written under train.result_save_path.  train.sampled_eval = N (run.py --sampled-eval [N]; no key
    of the reference's configs): once the pipeline has ended, the sampled-negatives protocol -- every test positive ranked
    among N sampled negatives (seed train.sampled_eval_seed, default 0), MRR and HitRate / NDCG at train.sampled_eval_ks
    (default [10]) (recommend.sampled_report) --, written under train.result_save_path.  train.conflict = N (run.py --conflict [N]; no key of the
    reference's configs): once the pipeline has ended, the domain-conflict report (conflict.report) over N batches per domain
    (0: whole passes), written to train.conflict_out or under train.result_save_path; result.json gains conflict_rate_all,
    mean_cosine_all, conflict_rate_meta and mean_cosine_meta.  train.isotonic = B (run.py --isotonic [B]; no key of the
    reference's configs): once the pipeline has ended, the isotonic report (isotonic.report) with B calibration bins, written
    to train.isotonic_out or under train.result_save_path; result.json gains isotonic.headline's keys (domain_brier,
    domain_mcb, ..., avg_mcb, weighted_mcb).  train.diversify = LAMBDA (run.py --diversify [LAMBDA]; no key of the reference's
    configs): once the pipeline has ended, every test user's top-N pool (train.diversify_pool, default min(128, 5 K)) is
    re-ranked to K items (recommend, or 10) by greedy Maximal Marginal Relevance (list_metrics.diversify_report), written to
    train.diversify_out or under train.result_save_path; result.json gains list_metrics.diversify_headline's keys.
    train.similar_items = K (run.py --similar-items [K]; no key of the reference's configs): once the pipeline has ended, every
    catalogue item's K exact cosine nearest neighbours on the item table of its domain's weights and the figures of that
    neighbour graph (neighbours.report), written to train.similar_items_out or under train.result_save_path; result.json
    gains neighbours.headline's keys (domain_<figure>, avg_<figure>, domain_affinity).  train.baselines = SHRINK (run.py
    --rank-eval [KS] --baselines [SHRINK]; no key of the reference's configs): behind the rank-eval report, MostPopular and
    ItemKNN (shrinkage SHRINK) under the same protocol beside the tower's figures (baselines.report), ItemKNN only for
    catalogues of at most train.baselines_max_items (default 16384) items, written to train.baselines_out or under
    train.result_save_path; result.json gains baselines.headline's keys (baselines_shrink, domain_<figure>_pop,
    domain_<figure>_itemknn, avg_<figure>_pop, avg_<figure>_itemknn, domain_overlap_pop, domain_overlap_itemknn,
    domain_cold_users, baselines_skipped)."""
    from .reports import EVAL_REPORTS
    from .utils import MultiDomainDataset
    rank, world = init_distributed()
    name = config["model"]["name"]
    lanes = n_lanes(config)
    if (world > 1 or lanes > 1) and not ("meta" in name and ("mamdr" in name or "domain_negotiation" in name or "reptile" in name)):
        raise NotImplementedError("multi-process / multi-lane runs shard the MAMDR (DN + DR), Domain Negotiation and Reptile "
                                  "wrappers only; got '%s'" % name)
    for e in EVAL_REPORTS:
        if config["train"].get(e.config_key) and (world > 1 or lanes > 1):
            raise NotImplementedError("train.%s (run.py %s): %s not gathered across processes or lanes "
                                      "(parallel.gather_domain_scalars carries loss and AUC only); run it with one process and "
                                      "train.lanes = 1" % (e.config_key, e.flag, e.refusal))
    if config["train"].get("baselines") is not None and (world > 1 or lanes > 1):       # (before rank_eval's: named as asked)
        raise NotImplementedError("train.baselines (run.py --baselines): the baselines are not ranked across processes "
                                  "or lanes (they are reported beside train.rank_eval's figures, which are not); run it with one "
                                  "process and train.lanes = 1")
    if config["train"].get("baselines") is not None and not config["train"].get("rank_eval"):
        raise ValueError("train.baselines needs train.rank_eval (run.py --rank-eval [KS] --baselines [SHRINK])")
    if config["train"].get("rank_eval") and (world > 1 or lanes > 1):
        raise NotImplementedError("train.rank_eval (run.py --rank-eval): the ranks are not computed across processes or lanes "
                                  "(the best phi_d slots are current only on their owners); run it with one process and "
                                  "train.lanes = 1")
    if config["train"].get("sampled_eval") and (world > 1 or lanes > 1):
        raise NotImplementedError("train.sampled_eval (run.py --sampled-eval): the slates are not ranked across processes or "
                                  "lanes (the best phi_d slots are current only on their owners); run it with one process and "
                                  "train.lanes = 1")
    if config["train"].get("conflict") is not None and (world > 1 or lanes > 1):
        raise NotImplementedError("train.conflict (run.py --conflict): the domain-conflict report is not computed across processes "
                                  "or lanes (one engine measures every domain's gradient at one point); run it with one process "
                                  "and train.lanes = 1")
    if config["train"].get("isotonic") is not None and (world > 1 or lanes > 1):
        raise NotImplementedError("train.isotonic (run.py --isotonic): the isotonic report is not computed across processes "
                                  "or lanes (the best phi_d slots are current only on their owners); run it with one process "
                                  "and train.lanes = 1")
    if config["train"].get("list_metrics") is not None and (world > 1 or lanes > 1):
        raise NotImplementedError("train.list_metrics (run.py --list-metrics): the list metrics are not computed across processes "
                                  "or lanes (the best phi_d slots are current only on their owners); run it with one process "
                                  "and train.lanes = 1")
    if config["train"].get("diversify") is not None and (world > 1 or lanes > 1):
        raise NotImplementedError("train.diversify (run.py --diversify): the diversified lists are not computed across processes "
                                  "or lanes (the best phi_d slots are current only on their owners); run it with one process "
                                  "and train.lanes = 1")
    if config["train"].get("similar_items") is not None and (world > 1 or lanes > 1):
        raise NotImplementedError("train.similar_items (run.py --similar-items): the neighbours are not computed across processes "
                                  "or lanes (the best phi_d slots are current only on their owners); run it with one process "
                                  "and train.lanes = 1")
    dataset = MultiDomainDataset(config["dataset"])
    if lanes > 1:
        # (under N processes the lanes of every rank are a slice of ONE world of N * lanes participants: a rank's DR queries
        # and DN sub-sequence are dealt on to its lanes, collectives = lane step + one inter-rank collective per process --
        # parallel.py, "RANKS x LANES")
        from . import parallel
        import os
        import torch
        if not torch.cuda.is_initialized():
            # every lane's stream on a hardware queue of its own (the HIP runtime reads this when it initialises; its
            # default of 4 queues is shared with torch's other streams: profiles/r05_lanes_bench.txt)
            os.environ.setdefault("GPU_MAX_HW_QUEUES", str(max(8, 2 * lanes)))
        # (the dataset is read-only: one copy for all lanes; every lane builds its own model = its own engine and stream)
        # (train.lane_sum_block: a test knob -- a one-process run of N * L lanes that adds up in the order of N processes of L
        # lanes, the bit-for-bit reference of the composed run: tests/test_abi_and_parallel.py)
        return parallel.LaneGroup(lanes, outer=(rank, world), sum_block=config["train"].get("lane_sum_block")).run(
            lambda lane: _run(config, dataset, engine_factory, on_model, rank * lanes + lane, recommend, recommend_out))[0]
    return _run(config, dataset, engine_factory, on_model, rank, recommend, recommend_out)


def _run(config, dataset, engine_factory, on_model, rank, recommend=None, recommend_out=None):
    name = config["model"]["name"]
    model = build_model(config, dataset, engine_factory)
    if on_model is not None:
        on_model(model)
    if "separate" in name:
        avg_loss, avg_auc, domain_loss, domain_auc = model.separate_train_val_test()
    else:
        model.train()
        print("Test Result: ")
        avg_loss, avg_auc, domain_loss, domain_auc = model.val_and_test("test")
    if "finetune" in name:
        model.load_model(model.checkpoint_path)      # the best checkpoint (kept on the device as well)
        print("Finetune: ")
        avg_loss, avg_auc, domain_loss, domain_auc = model.separate_train_val_test(init_parms=False)
    if rank == 0:
        saved = model.save_result(avg_loss, avg_auc, domain_loss, domain_auc)
        from . import recommend as rec
        if recommend:
            rec.report(model, int(recommend), recommend_out)
        if config["train"].get("rank_eval"):
            _, tower_ranks = rec.rank_report(model, config["train"]["rank_eval"])
            if config["train"].get("baselines") is not None:
                from . import baselines
                shrink = baselines.check_shrink(config["train"]["baselines"])
                _, reports = baselines.report(model, config["train"]["rank_eval"], int(recommend) if recommend else None,
                                              config["train"].get("baselines_out"), shrink,
                                              int(config["train"].get("baselines_max_items", baselines.DEFAULT_MAX_ITEMS)),
                                              tower=tower_ranks)
                _extend_result(saved, baselines.headline(reports, shrink))
        if config["train"].get("sampled_eval"):
            rec.sampled_report(model, int(config["train"]["sampled_eval"]), config["train"].get("sampled_eval_ks", [10]),
                               seed=int(config["train"].get("sampled_eval_seed", 0)))
        if config["train"].get("conflict") is not None:
            from . import conflict
            _, res = conflict.report(model, int(config["train"]["conflict"]), config["train"].get("conflict_out"))
            _extend_result(saved, conflict.headline(res))
        if config["train"].get("isotonic") is not None:
            from . import isotonic
            _, reports = isotonic.report(model, int(config["train"]["isotonic"]), config["train"].get("isotonic_out"))
            _extend_result(saved, isotonic.headline(reports))
        if config["train"].get("list_metrics") is not None:
            from . import list_metrics
            _, reports = list_metrics.report(model, int(config["train"]["list_metrics"]), config["train"].get("list_metrics_out"))
            _extend_result(saved, list_metrics.headline(reports))
        if config["train"].get("diversify") is not None:
            from . import list_metrics
            k, pool = list_metrics.check_pool(int(recommend) if recommend else list_metrics.DEFAULT_K,
                                              config["train"].get("diversify_pool"))
            lam = list_metrics.check_lambda(config["train"]["diversify"])
            _, reports = list_metrics.diversify_report(model, k, lam, pool, config["train"].get("diversify_out"))
            _extend_result(saved, list_metrics.diversify_headline(reports, lam, pool))
        if config["train"].get("similar_items") is not None:
            from . import neighbours
            _, reports = neighbours.report(model, int(config["train"]["similar_items"]), config["train"].get("similar_items_out"))
            _extend_result(saved, neighbours.headline(reports))
    return avg_loss, avg_auc, domain_loss, domain_auc


def _extend_result(saved, extra):
    """the keys of a post-run report into the result.json that save_result wrote (the report runs after it)."""
    path = os.path.join(saved, "result.json")
    with open(path) as f:
        result = json.load(f)
    result.update(extra)
    with open(path, "w") as f:
        json.dump(result, f)


def cli(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, help="Train config file", required=True)
    # (not an option of the reference's run.py: the sharded epoch on one GPU, see n_lanes)
    parser.add_argument("--lanes", type=int, default=None, help="run the sharded epoch on this many lanes of one process (train.lanes)")
    # (not options of the reference's run.py either: its pipeline ends at loss and AUC)
    parser.add_argument("--recommend", type=int, default=None, metavar="K",
                        help="after the run: top-K items per domain for its test users, with HitRate / Recall / NDCG @K")
    parser.add_argument("--recommend-out", type=str, default=None, metavar="FILE",
                        help=".npz the recommendations go to (default: under train.result_save_path)")
    parser.add_argument("--gauc", action="store_true",
                        help="also report the impression-weighted per-user AUC (GAUC) of every evaluation (train.report_gauc)")
    parser.add_argument("--exact-metrics", type=int, default=None, nargs="?", const=20, metavar="B",
                        help="also report the exact (tie-aware Mann-Whitney) AUC, the average precision and the calibration "
                             "over B equal-mass bins (default 20) of every evaluation (train.report_exact)")
    parser.add_argument("--auc-ci", type=int, default=None, nargs="?", const=1000, metavar="B",
                        help="also report the standard error and the 95 %% percentile interval of the exact AUC of every "
                             "evaluation from B bootstrap replicates (default 1000, 1 .. 65535) (train.report_auc_ci)")
    parser.add_argument("--auc-ci-unit", type=str, default=None, choices=("row", "user"),
                        help="what --auc-ci resamples: users (default; a user's rows are correlated) or rows (train.auc_ci_unit)")
    parser.add_argument("--auc-ci-seed", type=int, default=None, metavar="S",
                        help="the seed of --auc-ci's resampling weights (default 0) (train.auc_ci_seed)")
    parser.add_argument("--rank-eval", type=str, default=None, nargs="?", const="10,50,200", metavar="KS",
                        help="after the run: the exact rank of every test positive in its domain's whole catalogue, with MRR, mean "
                             "percentile and HitRate / Recall / NDCG at the comma list KS (default 10,50,200) (train.rank_eval)")
    parser.add_argument("--sampled-eval", type=int, default=None, nargs="?", const=99, metavar="N",
                        help="after the run: every test positive ranked among N sampled items its user never interacted with "
                             "(default 99), with MRR and HitRate / NDCG at --sampled-eval-ks (train.sampled_eval)")
    parser.add_argument("--sampled-eval-ks", type=str, default=None, metavar="KS",
                        help="the comma list of K for --sampled-eval (default 10) (train.sampled_eval_ks)")
    parser.add_argument("--conflict", type=int, default=None, nargs="?", const=8, metavar="N",
                        help="after the run: the domain-conflict report -- cosines between the domains' gradients over N batches "
                             "per domain (default 8; 0: whole passes), per tensor, with the share of conflicting pairs "
                             "(train.conflict)")
    parser.add_argument("--conflict-out", type=str, default=None, metavar="FILE",
                        help=".npz the domain-conflict report goes to (default: under train.result_save_path)")
    parser.add_argument("--isotonic", type=int, default=None, nargs="?", const=20, metavar="B",
                        help="after the run: isotonic recalibration of every domain -- fitted on its val split, applied to its "
                             "test split -- with Brier / log loss / ECE / PCOC (B equal-mass bins, default 20, 1 .. 4096) before "
                             "and after, and the CORP decomposition of the test Brier score (train.isotonic)")
    parser.add_argument("--isotonic-out", type=str, default=None, metavar="FILE",
                        help=".npz the isotonic fits go to (default: under train.result_save_path)")
    parser.add_argument("--list-metrics", type=int, default=None, nargs="?", const=-1, metavar="K",
                        help="after the run: what every domain's top-K lists are made of -- catalogue coverage, Gini and entropy "
                             "of exposure, novelty, average popularity, tail share, personalisation and intra-list diversity "
                             "(K 1 .. 128; default: --recommend's K, or 10) (train.list_metrics)")
    parser.add_argument("--list-metrics-out", type=str, default=None, metavar="FILE",
                        help=".npz the list metrics go to (default: under train.result_save_path)")
    parser.add_argument("--diversify", type=float, default=None, nargs="?", const=0.7, metavar="LAMBDA",
                        help="after the run: every test user's top-N pool re-ranked to K items (--recommend's K, or 10) by greedy "
                             "Maximal Marginal Relevance, lambda * relevance - (1 - lambda) * (largest cosine with a pick so far) "
                             "(LAMBDA 0 .. 1, default 0.7), with HitRate / NDCG and the list metrics of both sides (train.diversify)")
    parser.add_argument("--diversify-pool", type=int, default=None, metavar="N",
                        help="the pool --diversify picks from: each user's top N (K .. 128; default min(128, 5 K)) "
                             "(train.diversify_pool)")
    parser.add_argument("--diversify-out", type=str, default=None, metavar="FILE",
                        help=".npz the diversified lists go to (default: under train.result_save_path)")
    parser.add_argument("--similar-items", type=int, default=None, nargs="?", const=10, metavar="K",
                        help="after the run: every catalogue item's K exact cosine nearest neighbours on the item table, per "
                             "domain, with mean similarity, hubness, orphan share and reciprocity of the neighbour graph and the "
                             "embedding-space affinity between the domains (K 1 .. 128, default 10) (train.similar_items)")
    parser.add_argument("--similar-items-out", type=str, default=None, metavar="FILE",
                        help=".npz the neighbour lists go to (default: under train.result_save_path)")
    parser.add_argument("--baselines", type=float, default=None, nargs="?", const=10.0, metavar="SHRINK",
                        help="with --rank-eval: MostPopular and ItemKNN (cosine over co-occurrence counts, shrinkage SHRINK 0 .. 2^20, "
                             "default 10) under the same protocol, beside the tower's figures; with --recommend K also the "
                             "overlap of their top-K lists with the tower's (train.baselines)")
    parser.add_argument("--baselines-out", type=str, default=None, metavar="FILE",
                        help=".npz the baselines' ranks and lists go to (default: under train.result_save_path)")
    parser.add_argument("--baselines-max-items", type=int, default=None, metavar="N",
                        help="the largest catalogue ItemKNN is computed for (its co-occurrence matrix takes 4 N^2 bytes; default "
                             "16384, at most 65535); a larger domain gets MostPopular only and is named (train.baselines_max_items)")
    args = parser.parse_args(argv)
    with open(args.config, "r") as f:
        config = json.load(f)
    if args.lanes is not None:
        config["train"]["lanes"] = args.lanes
    if args.gauc:
        config["train"]["report_gauc"] = True
    if args.exact_metrics is not None:
        if not 1 <= args.exact_metrics <= 4096:
            parser.error("--exact-metrics B: B calibration bins, 1 .. 4096")
        config["train"]["report_exact"] = args.exact_metrics
    if args.auc_ci is not None:
        if not 1 <= args.auc_ci <= 65535:
            parser.error("--auc-ci B: B bootstrap replicates, 1 .. 65535")
        config["train"]["report_auc_ci"] = args.auc_ci
    for flag, value, key in (("--auc-ci-unit", args.auc_ci_unit, "auc_ci_unit"), ("--auc-ci-seed", args.auc_ci_seed, "auc_ci_seed")):
        if value is not None:
            if not config["train"].get("report_auc_ci"):
                parser.error("%s needs --auc-ci [B] (or train.report_auc_ci in the config)" % flag)
            config["train"][key] = value
    if args.auc_ci is not None:          # the flag's defaults, spelled out in the saved config
        config["train"].setdefault("auc_ci_unit", "user")
        config["train"].setdefault("auc_ci_seed", 0)
    if args.rank_eval is not None:
        config["train"]["rank_eval"] = [int(k) for k in args.rank_eval.split(",")]
    if args.sampled_eval is not None:
        if args.sampled_eval < 1:
            parser.error("--sampled-eval N: N negatives per positive, at least 1")
        config["train"]["sampled_eval"] = args.sampled_eval
    if args.sampled_eval_ks is not None:
        if not config["train"].get("sampled_eval"):
            parser.error("--sampled-eval-ks KS needs --sampled-eval [N] (or train.sampled_eval in the config)")
        config["train"]["sampled_eval_ks"] = [int(k) for k in args.sampled_eval_ks.split(",")]
    if args.conflict is not None:
        if args.conflict < 0:
            parser.error("--conflict N: N batches per domain, 0 for whole passes")
        config["train"]["conflict"] = args.conflict
    if args.conflict_out is not None:
        config["train"]["conflict_out"] = args.conflict_out
    if args.isotonic is not None:
        if not 1 <= args.isotonic <= 4096:
            parser.error("--isotonic B: B calibration bins, 1 .. 4096")
        config["train"]["isotonic"] = args.isotonic
    if args.isotonic_out is not None:
        config["train"]["isotonic_out"] = args.isotonic_out
    if args.list_metrics is not None:
        k = args.list_metrics if args.list_metrics != -1 else (args.recommend or 10)          # (no value: --recommend's K, or 10)
        if not 1 <= k <= 128:
            parser.error("--list-metrics K: lists of K items, 1 .. 128")
        config["train"]["list_metrics"] = k
    if args.list_metrics_out is not None:
        config["train"]["list_metrics_out"] = args.list_metrics_out
    if args.diversify is not None:
        if not 0.0 <= args.diversify <= 1.0:          # (NaN fails both comparisons)
            parser.error("--diversify LAMBDA: the weight of relevance, 0 .. 1")
        config["train"]["diversify"] = args.diversify
    if args.diversify_pool is not None:
        if config["train"].get("diversify") is None:
            parser.error("--diversify-pool N needs --diversify [LAMBDA] (or train.diversify in the config)")
        config["train"]["diversify_pool"] = args.diversify_pool
    if args.diversify_out is not None:
        config["train"]["diversify_out"] = args.diversify_out
    if args.similar_items is not None:
        if not 1 <= args.similar_items <= 128:
            parser.error("--similar-items K: K neighbours per item, 1 .. 128")
        config["train"]["similar_items"] = args.similar_items
    if args.similar_items_out is not None:
        config["train"]["similar_items_out"] = args.similar_items_out
    if args.baselines is not None:
        if not 0.0 <= args.baselines <= 2.0 ** 20:          # (NaN fails both comparisons)
            parser.error("--baselines SHRINK: the shrinkage of the ItemKNN similarity, 0 .. 2^20")
        config["train"]["baselines"] = args.baselines
    for flag, value, key in (("--baselines-out", args.baselines_out, "baselines_out"),
                             ("--baselines-max-items", args.baselines_max_items, "baselines_max_items")):
        if value is not None:
            if config["train"].get("baselines") is None:
                parser.error("%s needs --baselines [SHRINK] (or train.baselines in the config)" % flag)
            config["train"][key] = value
    if args.baselines_max_items is not None and not 1 <= args.baselines_max_items <= 65535:
        parser.error("--baselines-max-items N: items, 1 .. 65535")
    if config["train"].get("baselines") is not None:
        if not config["train"].get("rank_eval"):
            parser.error("--baselines needs --rank-eval [KS] (or train.rank_eval in the config): the baselines are reported "
                         "under its protocol, beside its figures")
        if args.recommend is not None and not 1 <= args.recommend <= 128:
            parser.error("--baselines with --recommend K: lists of K items, 1 .. 128")
    if config["train"].get("diversify") is not None:
        k = args.recommend or 10
        n = config["train"].get("diversify_pool")
        if not 1 <= k <= 128 or (n is not None and not k <= int(n) <= 128):
            parser.error("--diversify: K = %d (--recommend's, or 10) of a pool of N items, K <= N <= 128" % k)
    if args.recommend is None:
        return main(config)
    return main(config, recommend=args.recommend, recommend_out=args.recommend_out)
