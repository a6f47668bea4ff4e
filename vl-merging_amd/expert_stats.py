#!/usr/bin/env python
"""`python expert_stats.py --ckpt IN [--central C | --raw] [--trunc-rms R] --report R.json with <named configs> key=value ...`:
how far apart are the modality experts of an all_moe checkpoint, and will merging them work?

Per tensor and over the whole checkpoint, between every pair of the experts "v", "l" and "vl": L2 distance, cosine similarity,
soft sign dissimilarity, its truncated form and the sign-conflict rate (merge.expert_stats; the rule: include/vlm_hip.h), computed
on the GPU in one pass over the checkpoint.  Nothing is merged and no checkpoint is written: the report is the output, and what one
picks merge_ckpt.py's --density, --drop and --lambda from.  The words after the options are a config in run.py's grammar
(`config.parse_cli`): they decide `vlffn_start_layer_index`, `only_activate_used_experts`, `loss_names`, `central_weight`.

  --central C      the central (ufo) checkpoint: the statistics are those of the task vectors W_m - central
                   (default: central_weight of the config)
  --raw            the experts' weights as they are; no central checkpoint is read
  --trunc-rms R    the truncated statistics count an element only where an entry reaches R times its tensor's root mean square;
                   costs a second pass over the checkpoint
  --report R.json  {"raw", "trunc_rms", "tensors": [one row per tensor], "summary": {pair: sums and measures}}
"""
import argparse
import importlib
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(prog="expert_stats.py", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--ckpt", required=True, help="all_moe checkpoint (a Lightning .ckpt or a bare state_dict file)")
    which = p.add_mutually_exclusive_group()
    which.add_argument("--central", default=None, help="central (ufo) checkpoint; default: central_weight of the config")
    which.add_argument("--raw", action="store_true", help="statistics of the weights themselves, not of the task vectors")
    p.add_argument("--trunc-rms", dest="trunc_rms", type=float, default=None,
                   help="threshold of the truncated statistics in units of each tensor's root mean square (> 0)")
    p.add_argument("--report", required=True, help="write the JSON report here")
    p.add_argument("config", nargs="*", help="with <named configs> key=value ... (as for run.py)")
    return p


def parse_args(argv):
    """(options, config): no device is touched."""
    args = build_parser().parse_args(argv)
    if args.trunc_rms is not None and not (args.trunc_rms > 0.0 and math.isfinite(args.trunc_rms)):
        raise ValueError("--trunc-rms must be a positive finite number, got %r" % (args.trunc_rms,))
    ge.import_package()
    cfg = importlib.import_module("vl_merging_amd.vilt.config").parse_cli(args.config)
    return args, cfg


def main(argv):
    args, cfg = parse_args(argv)
    merge = importlib.import_module("vl_merging_amd.merge")
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    sd = ckpt.load_ckpt(args.ckpt)
    central = ckpt.load_file(args.central) if args.central else None
    res = merge.expert_stats(sd, cfg, central_weight=central, raw=args.raw, trunc_rms=args.trunc_rms)
    with open(args.report, "w") as f:
        json.dump(res, f, indent=1)
    print("expert_stats: %s -> %s (%d tensors)" % (args.ckpt, args.report, len(res["tensors"])))
    for name, s in res["summary"].items():
        print("  %-5s l2 %.6g  cosine %s  ssd %s  conflict rate %s" % (name, s["l2"], s["cosine"], s["ssd"], s["conflict_rate"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
