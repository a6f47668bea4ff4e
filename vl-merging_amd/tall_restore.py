#!/usr/bin/env python
"""`python tall_restore.py --unified U.ckpt --central ufo.ckpt --masks masks.pt --out all_moe.ckpt with <named configs> key=value ...`:
rebuild the modality experts of an all_moe checkpoint from ufo-sized data.

The unified checkpoint is what `merge_ckpt.py --method consensus --consensus-k 0 --lambda 1 --masks-out masks.pt` wrote: the central
tensors plus the summed task vectors.  With the central checkpoint and the packed TALL masks (one bit per element and expert) every
expert's tensor comes back as `bit ? unified : central`, which is central + mask * (the summed task vector): the reconstruction of
Wang et al. 2024 (merge.tall_restore; the rule: include/vlm_hip.h), computed on the GPU in one launch.  Two fp32 checkpoints and
S bits per element stand in for S fp32 experts.
A masks file of `merge_ckpt.py --method emr --lambda 1 --masks-out masks.pt` (format emr-masks-1) is read as well: the unified
checkpoint is then the EMR merge, the masks are its agreement masks, and every expert's tensor comes back as
`central + rescaler * (bit ? unified - central : 0)` with the file's one rescaler per tensor and expert (merge.emr_restore).  The
file's `format` decides which of the two it is.  The words after the options are a config in run.py's grammar
(`config.parse_cli`): they decide `vlffn_start_layer_index`, `only_activate_used_experts`, `loss_names`, `central_weight`.

  --unified U.ckpt   the k = 0, lambda = 1 consensus merge, or the lambda = 1 EMR merge (a Lightning .ckpt or a bare state_dict file)
  --central C        the central (ufo) checkpoint (default: central_weight of the config)
  --masks M.pt       the file merge_ckpt.py --masks-out wrote: {"format": "tall-masks-1", "tall_lambda", "k", "masks": {source key: words}}
                     or {"format": "emr-masks-1", "masks": {source key: words}, "rescalers": {source key: float}}
  --out OUT          the all_moe checkpoint to write: a `{"state_dict": ...}` file of CPU tensors
"""
import argparse
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

MASKS_FORMAT = "tall-masks-1"
EMR_FORMAT = "emr-masks-1"


def build_parser():
    p = argparse.ArgumentParser(prog="tall_restore.py", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--unified", required=True, help="the unified checkpoint: consensus with k = 0 and lambda = 1")
    p.add_argument("--central", default=None, help="central (ufo) checkpoint; default: central_weight of the config")
    p.add_argument("--masks", required=True, help="the masks file merge_ckpt.py --masks-out wrote")
    p.add_argument("--out", required=True, help="all_moe checkpoint to write")
    p.add_argument("config", nargs="*", help="with <named configs> key=value ... (as for run.py)")
    return p


def parse_args(argv):
    """(options, config): no device is touched."""
    args = build_parser().parse_args(argv)
    ge.import_package()
    cfg = importlib.import_module("vl_merging_amd.vilt.config").parse_cli(args.config)
    return args, cfg


def read_masks_file(path):
    """(format, masks, rescalers | None) of a masks file of either format; ValueError if it is neither."""
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    data = ckpt.load_file(path)
    fmt = data.get("format") if isinstance(data, dict) else None
    ok = fmt in (MASKS_FORMAT, EMR_FORMAT) and isinstance(data.get("masks"), dict)
    if not ok or (fmt == EMR_FORMAT and not isinstance(data.get("rescalers"), dict)):
        raise ValueError("%s is neither a %s nor an %s file (format: %r)" % (path, MASKS_FORMAT, EMR_FORMAT, fmt))
    return fmt, data["masks"], data["rescalers"] if fmt == EMR_FORMAT else None


def read_masks(path):
    """The `masks` dictionary of a tall-masks-1 file; ValueError if it is not one."""
    fmt, masks, _ = read_masks_file(path)
    if fmt != MASKS_FORMAT:
        raise ValueError("%s is not a %s file" % (path, MASKS_FORMAT))
    return masks


def main(argv):
    import torch
    args, cfg = parse_args(argv)
    merge = importlib.import_module("vl_merging_amd.merge")
    ckpt = importlib.import_module("vl_merging_amd.checkpoint")
    fmt, masks, rescalers = read_masks_file(args.masks)
    sd = ckpt.load_ckpt(args.unified)
    central = ckpt.load_file(args.central) if args.central else None
    if fmt == EMR_FORMAT:
        out = merge.emr_restore(sd, masks, rescalers, cfg, central_weight=central)
    else:
        out = merge.tall_restore(sd, masks, cfg, central_weight=central)
    torch.cuda.synchronize()
    torch.save({"state_dict": {k: v.detach().to("cpu") for k, v in out.items()}}, args.out)
    print("tall_restore: %s + %s -> %s (%d masks, %d tensors)" % (args.unified, args.masks, args.out, len(masks), len(out)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
