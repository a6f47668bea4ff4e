#!/usr/bin/env python
"""`python merge_ckpt.py --method {interp,taskvec,ties,dare,breadcrumbs,della,stock,sce,slerp,karcher,consensus,emr,isoc,tsvm,wudi} --ckpt IN --out OUT [...] with <named configs> key=value ...`:
merge the modality experts of an all_moe checkpoint on the GPU and write the merged (ufo) checkpoint to disk.

The reference merges only while a model loads (src/vilt/modules/vilt_module.py:284-305 calls merge_weights /
sum_task_vectors / regmean on the state_dict it has just read); a merged checkpoint on disk is what one hands on, so this tool
runs the same merges (merge.merge_weights, merge.sum_task_vectors), TIES (merge.ties_merge), DARE (merge.dare_merge), Model
Breadcrumbs (merge.band_merge), DELLA (merge.della_merge), Model Stock (merge.stock_merge), SCE (merge.sce_merge), the spherical merge (merge.sphere_merge) and
the consensus merge with TALL masks (merge.consensus_merge) and EMR-Merging (merge.emr_merge; none of the nine has a reference site) outside a model.  The words after the options are a config in run.py's grammar (`config.parse_cli`): they decide
`vlffn_start_layer_index`, `only_activate_used_experts`, `loss_names`, `merge_ratio`, `sum_lambda`, `central_weight`.

  --method interp    merge_weights      (--ratio overrides merge_ratio)
  --method taskvec   sum_task_vectors   (--lambda overrides sum_lambda; --central or central_weight=<path> is the ufo checkpoint)
  --method ties      ties_merge         (--density, --lambda, --central as above)
  --method dare      dare_merge         (--drop, --seed, --dare-mode {linear,ties}, --no-rescale, --lambda, --central as above)
  --method breadcrumbs  band_merge      (--density = the band kept, --gamma = the share of largest entries dropped above it,
                                         --band-mode {linear,ties}, --lambda, --central as above)
  --method della     della_merge        (--density +- --epsilon = the keep probability of a row's largest / smallest entry,
                                         --seed, --della-mode {linear,ties}, --no-rescale, --lambda, --central as above)
  --method stock     stock_merge        (--central as above; the method has no hyper-parameter: --lambda, --density and the rest are
                                         ignored, as they are for interp)
  --method sce       sce_merge          (--density = the share of elements selected by their variance across the experts;
                                         --lambda, --central as above)
  --method slerp     sphere_merge       (`karcher` is the same method: SLERP is its two-source case.  --sphere-on weights merges
                                         the experts' weights as interp does, with --ratio; --sphere-on delta merges their task
                                         vectors, with --lambda and --central as above; --sphere-rows: one mean per row)
  --method consensus consensus_merge    (--tall-lambda = how large an expert's entry must be against the other experts' sum to be
                                         relevant to it, --consensus-k = how many experts must find an element relevant,
                                         --masks-out M.pt = also write the packed TALL masks, from which tall_restore.py
                                         rebuilds the experts; --lambda, --central as above)
  --method emr       emr_merge          (elect a sign, take the largest agreeing magnitude; tuning-free: --lambda and --central as
                                         above are all it reads.  --masks-out M.pt = also write {format: emr-masks-1, masks,
                                         rescalers}: one agreement bit per element and expert and one scalar per tensor and
                                         expert, from which tall_restore.py rebuilds the experts -- merge with --lambda 1 for that)
  --method isoc      isoc.isoc_merge    (Iso-C: every weight matrix takes the SUM of its task vectors with the singular values
                                         flattened to their mean, every other tensor the mean task vector; tuning-free: --lambda
                                         and --central as above are all it reads)
  --method tsvm      tsvm.tsvm_merge    (TSV-M: every weight matrix keeps each expert's leading min(m, n) // S singular triplets and
                                         orthogonalises the kept subspaces across the experts before recombining them, through a
                                         float64 Jacobi SVD; every other tensor the mean task vector; tuning-free: --lambda and
                                         --central as above are all it reads)
  --method wudi      wudi.wudi_merge    (WUDI-Merging: every weight matrix takes --wudi-iters Adam steps at --wudi-lr, in float64,
                                         on sum_i ||(X - tau_i) tau_i^T||_F^2 / ||tau_i||_F^2 from the sum of its task vectors
                                         tau_i -- data-free: the task vectors' own Gram matrices stand in for RegMean's --, every
                                         other tensor the mean task vector; --lambda and --central as above)
  --report R.json    one entry per merged tensor (ties: n, K, threshold, kept per source, conflict, empty;
                     dare: n, keep_below, kept per source, conflict, empty;
                     breadcrumbs: n, k_hi, k_lo, both thresholds, kept and outlier per source, conflict, empty;
                     della: n, keep_lo, keep_hi, row_len, kept per source, conflict, empty;
                     stock: n, sq per source, dot and cosine per pair, the mean cosine, t, scale and its bits;
                     sce: n, K, the variance threshold, kept, sq and weight per source, tot, conflict, empty;
                     slerp: n, row_len, weights, lam and, per tensor, sq, dot per pair, coef64, coef32 and its bits, rho, resid,
                     status -- per row instead: rows, rows_linear, rows_zero, resid_max;
                     consensus: n, op, k, tall_lambda, kept per source, selected, empty;
                     emr: n, op, kept per source, zero, conflict, abs_sum, uni_sum and rescale per source;
                     isoc, per matrix: n, shape, transposed, S, fro, nuclear, sigma_mean, steps, last_step, converged;
                     tsvm, per matrix: n, shape, transposed, S, k, sweeps and converged of every SVD taken ({tau: per source, U, V}),
                     s_max, s_kept_min, s_dropped_max and energy_kept per source, dropped ({U, V}: polar directions dropped);
                     wudi, per matrix: n, shape, S, iters, lr, sq per source, loss_first, loss_last)

The output is a `{"state_dict": ...}` file of CPU tensors: checkpoint.load_ckpt and the reference's torch.load read it.
"""
import argparse
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

METHODS = ("interp", "taskvec", "ties", "dare", "breadcrumbs", "della", "stock", "sce", "slerp", "karcher", "consensus", "emr", "isoc", "tsvm", "wudi")


def build_parser():
    p = argparse.ArgumentParser(prog="merge_ckpt.py", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--method", choices=METHODS, required=True)
    p.add_argument("--ckpt", required=True, help="all_moe checkpoint (a Lightning .ckpt or a bare state_dict file)")
    p.add_argument("--out", required=True, help="merged checkpoint to write")
    p.add_argument("--central", default=None, help="central (ufo) checkpoint of taskvec / ties / dare / breadcrumbs / della / stock / sce / slerp on delta; default: central_weight of the config")
    p.add_argument("--density", type=float, default=0.2,
                   help="ties / breadcrumbs: fraction of each task vector kept, in (0, 1]; della: the mean keep probability; "
                        "sce: fraction of the elements selected by their variance across the experts, in (0, 1]")
    p.add_argument("--lambda", dest="lam", type=float, default=None, help="taskvec / ties / dare / breadcrumbs / della / sce / slerp on delta: overrides sum_lambda")
    p.add_argument("--drop", type=float, default=0.9, help="dare: probability of dropping a task-vector entry, in [0, 1)")
    p.add_argument("--seed", type=int, default=0, help="dare / della: seed of the mask (64 bits)")
    p.add_argument("--dare-mode", dest="dare_mode", choices=("linear", "ties"), default="linear",
                   help="dare: sum the rescaled survivors, or elect a sign and average them as TIES does")
    p.add_argument("--no-rescale", dest="rescale", action="store_false", help="dare / della: do not scale the survivors by the reciprocal of their keep probability")
    p.add_argument("--gamma", type=float, default=0.01,
                   help="breadcrumbs: fraction of each task vector's largest entries dropped as outliers, in [0, 1)")
    p.add_argument("--band-mode", dest="band_mode", choices=("linear", "ties"), default="linear",
                   help="breadcrumbs: sum the band, or elect a sign and average it as TIES does")
    p.add_argument("--epsilon", type=float, default=0.1,
                   help="della: the keep probability runs from density - epsilon (a row's smallest entry) to density + epsilon "
                        "(its largest); needs 0 < density - epsilon and density + epsilon <= 1")
    p.add_argument("--della-mode", dest="della_mode", choices=("linear", "ties"), default="linear",
                   help="della: sum the rescaled survivors, or elect a sign and average them as TIES does")
    p.add_argument("--ratio", type=float, default=None, help="interp / slerp: overrides merge_ratio")
    p.add_argument("--sphere-on", dest="sphere_on", choices=("weights", "delta"), default="weights",
                   help="slerp / karcher: merge the experts' weights themselves (no central checkpoint), or their task vectors")
    p.add_argument("--sphere-rows", dest="sphere_rows", action="store_true",
                   help="slerp / karcher: one spherical mean per row of a tensor (a vector is one row) instead of one per tensor")
    p.add_argument("--tall-lambda", dest="tall_lambda", type=float, default=0.4,
                   help="consensus: an expert's entry is relevant to it iff |entry| >= tall_lambda * |the other experts' sum|; >= 0")
    p.add_argument("--consensus-k", dest="consensus_k", type=int, default=2,
                   help="consensus: keep an element iff at least k experts find it relevant (a layer with S experts uses min(k, S)); "
                        "0 is plain task arithmetic")
    p.add_argument("--wudi-iters", dest="wudi_iters", type=int, default=300, help="wudi: Adam steps per weight matrix, >= 1")
    p.add_argument("--wudi-lr", dest="wudi_lr", type=float, default=1e-5, help="wudi: Adam's learning rate, > 0")
    p.add_argument("--masks-out", dest="masks_out", default=None,
                   help="consensus: write {format: tall-masks-1, tall_lambda, k, masks: {source key: int32 words}} here; "
                        "emr: write {format: emr-masks-1, masks: {source key: int32 words}, rescalers: {source key: float}} here")
    p.add_argument("--report", default=None, help="write a JSON report here")
    p.add_argument("config", nargs="*", help="with <named configs> key=value ... (as for run.py)")
    return p


def parse_args(argv):
    """(options, config): no device is touched."""
    args = build_parser().parse_args(argv)
    ge.import_package()
    cfgmod = importlib.import_module("vl_merging_amd.vilt.config")
    cfg = cfgmod.parse_cli(args.config)
    if args.lam is not None:
        cfg["sum_lambda"] = args.lam
    if args.ratio is not None:
        cfg["merge_ratio"] = args.ratio
    if args.method == "ties" and not (0.0 < args.density <= 1.0):
        raise ValueError("TIES density must lie in (0, 1], got %r" % (args.density,))
    if args.method == "sce" and not (0.0 < args.density <= 1.0):
        raise ValueError("SCE density must lie in (0, 1], got %r" % (args.density,))
    if args.method == "dare":
        importlib.import_module("vl_merging_amd.merge").dare_keep_below(args.drop)  # the one statement of the rule; ValueError
        if not 0 <= args.seed < 2 ** 64:
            raise ValueError("DARE seed must fit 64 bits, got %r" % (args.seed,))
    if args.method == "breadcrumbs":
        importlib.import_module("vl_merging_amd.merge").band_ranks(1, args.density, args.gamma)  # the one statement; ValueError
    if args.method == "della":
        importlib.import_module("vl_merging_amd.merge").della_window(args.density, args.epsilon)  # the one statement; ValueError
        if not 0 <= args.seed < 2 ** 64:
            raise ValueError("DELLA seed must fit 64 bits, got %r" % (args.seed,))
    if args.method == "wudi":
        if args.wudi_iters < 1:
            raise ValueError("WUDI takes --wudi-iters >= 1, got %r" % (args.wudi_iters,))
        if not (args.wudi_lr > 0.0 and args.wudi_lr < float("inf")):
            raise ValueError("WUDI takes a finite --wudi-lr > 0, got %r" % (args.wudi_lr,))
    if args.method == "consensus":
        merge = importlib.import_module("vl_merging_amd.merge")
        merge.tall_threshold(args.tall_lambda)  # the one statement of each rule; ValueError
        merge.consensus_k(args.consensus_k)
    elif args.method != "emr" and args.masks_out is not None:
        raise ValueError("--masks-out belongs to --method consensus or emr (got %s)" % args.method)
    return args, cfg


def merge_state(method, sd, cfg, central=None, density=0.2, report=None, dare=None, band=None, della=None, sphere=None,
                consensus=None, emr=None, wudi=None):
    """The merged state_dict (device tensors for merged keys, the input's objects for the rest).  `dare`: the keyword arguments of
    merge.dare_merge (drop, seed, mode, rescale); `band`: those of merge.band_merge beside the density (gamma, mode); `della`: those of
    merge.della_merge beside the density (epsilon, seed, mode, rescale); `sphere`: those of merge.sphere_merge (on, rows); `consensus`: those of merge.consensus_merge (tall_lambda, k, masks_out); `emr`: those of merge.emr_merge (masks_out, rescalers_out); `wudi`: those of wudi.wudi_merge (iters, lr)."""
    merge = importlib.import_module("vl_merging_amd.merge")
    if method == "interp":
        out = merge.merge_weights(sd, cfg)
    elif method == "taskvec":
        out = merge.sum_task_vectors(sd, cfg, central_weight=central)
    elif method == "dare":
        rows = []
        out = merge.dare_merge(sd, cfg, central_weight=central, report_out=rows, **(dare or {}))
        if report is not None:
            report.extend(rows)
    elif method == "della":
        rows = []
        out = merge.della_merge(sd, cfg, central_weight=central, density=density, report_out=rows, **(della or {}))
        if report is not None:
            report.extend(rows)
    elif method == "stock":
        rows = []
        out = merge.stock_merge(sd, cfg, central_weight=central, report_out=rows)
        if report is not None:
            report.extend(rows)
    elif method == "sce":
        rows = []
        out = merge.sce_merge(sd, cfg, central_weight=central, density=density, report_out=rows)
        if report is not None:
            report.extend(rows)
    elif method in ("slerp", "karcher"):
        rows = []
        out = merge.sphere_merge(sd, cfg, central_weight=central, report_out=rows, **(sphere or {}))
        if report is not None:
            report.extend(rows)
    elif method == "consensus":
        rows = []
        out = merge.consensus_merge(sd, cfg, central_weight=central, report_out=rows, **(consensus or {}))
        if report is not None:
            report.extend(rows)
    elif method == "emr":
        rows = []
        out = merge.emr_merge(sd, cfg, central_weight=central, report_out=rows, **(emr or {}))
        if report is not None:
            report.extend(rows)
    elif method == "isoc":
        rows = []
        out = importlib.import_module("vl_merging_amd.isoc").isoc_merge(sd, cfg, central_weight=central, report_out=rows)
        if report is not None:
            report.extend(rows)
    elif method == "tsvm":
        rows = []
        out = importlib.import_module("vl_merging_amd.tsvm").tsvm_merge(sd, cfg, central_weight=central, report_out=rows)
        if report is not None:
            report.extend(rows)
    elif method == "wudi":
        rows = []
        out = importlib.import_module("vl_merging_amd.wudi").wudi_merge(sd, cfg, central_weight=central, report_out=rows, **(wudi or {}))
        if report is not None:
            report.extend(rows)
    elif method == "breadcrumbs":
        rows = []
        out = merge.band_merge(sd, cfg, central_weight=central, density=density, report_out=rows, **(band or {}))
        if report is not None:
            report.extend(rows)
    else:
        rows = []
        out = merge.ties_merge(sd, cfg, central_weight=central, density=density, report_out=rows)
        if report is not None:
            report.extend(rows)
    if report is not None:
        # a merged key is one the merge made a tensor for: absent from the input, or present but replaced (every merge here
        # allocates fresh outputs and hands pass-through keys back as the input's own objects)
        seen = {r["dst"] for r in report}
        report.extend({"dst": k, "n": v.numel()} for k, v in out.items() if k not in seen and sd.get(k) is not v)
    return out


def main(argv):
    import torch
    args, cfg = parse_args(argv)
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    sd = ckpt.load_ckpt(args.ckpt)
    central = ckpt.load_file(args.central) if args.central else None
    report = [] if args.report else None
    is_dare, is_band, is_della = args.method == "dare", args.method == "breadcrumbs", args.method == "della"
    is_sphere = args.method in ("slerp", "karcher")
    is_tall = args.method == "consensus"
    is_emr = args.method == "emr"
    masks = {} if (is_tall or is_emr) and args.masks_out else None
    rescalers = {} if masks is not None and is_emr else None
    has_density = args.method in ("ties", "sce") or is_band or is_della
    out = merge_state(args.method, sd, cfg, central=central, density=args.density, report=report,
                      dare=dict(drop=args.drop, seed=args.seed, mode=args.dare_mode, rescale=args.rescale),
                      band=dict(gamma=args.gamma, mode=args.band_mode),
                      della=dict(epsilon=args.epsilon, seed=args.seed, mode=args.della_mode, rescale=args.rescale),
                      sphere=dict(on=args.sphere_on, rows=args.sphere_rows),
                      consensus=dict(tall_lambda=args.tall_lambda, k=args.consensus_k, masks_out=masks),
                      emr=dict(masks_out=masks, rescalers_out=rescalers),
                      wudi=dict(iters=args.wudi_iters, lr=args.wudi_lr))
    torch.cuda.synchronize()
    torch.save({"state_dict": {k: v.detach().to("cpu") for k, v in out.items()}}, args.out)
    if rescalers is not None:
        torch.save({"format": "emr-masks-1", "masks": {k: v.to("cpu") for k, v in masks.items()}, "rescalers": rescalers}, args.masks_out)
    elif masks is not None:
        torch.save({"format": "tall-masks-1", "tall_lambda": args.tall_lambda, "k": args.consensus_k,
                    "masks": {k: v.to("cpu") for k, v in masks.items()}}, args.masks_out)
    if args.report:
        with open(args.report, "w") as f:
            json.dump({"method": args.method, "density": args.density if has_density else None,
                       "drop": args.drop if is_dare else None, "seed": args.seed if is_dare or is_della else None,
                       "dare_mode": args.dare_mode if is_dare else None,
                       "gamma": args.gamma if is_band else None, "band_mode": args.band_mode if is_band else None,
                       "epsilon": args.epsilon if is_della else None, "della_mode": args.della_mode if is_della else None,
                       "rescale": args.rescale if is_dare or is_della else None,
                       "sphere_on": args.sphere_on if is_sphere else None, "sphere_rows": args.sphere_rows if is_sphere else None,
                       "tall_lambda": args.tall_lambda if is_tall else None, "consensus_k": args.consensus_k if is_tall else None,
                       "sum_lambda": cfg["sum_lambda"], "merge_ratio": cfg["merge_ratio"], "tensors": report}, f, indent=1)
    print("merge_ckpt: %s -> %s (%s, %d tensors)" % (args.ckpt, args.out, args.method, len(out)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
