"""``python -m scale_imagenet_amd.main``: evaluate an ImageNet-style folder, the counterpart of ``python3 main.py``.

The reference's driver (main.py) builds TT_vf_19lv3_imgnet_small, loads ``./ckpt/last.pth``, runs ``test()`` over
``<data_dir>/val`` and prints ``Acc.. <top-1> <top-5>`` (main.py:196-284).  This command does the same through the
project's own path: the files' bytes go to the device (``FileBytesFolder`` + ``collate_jpeg``), are decoded, resized,
cropped and classified there (``evaluate(..., metrics="device")``), and only four numbers per rank come back.  The
flags carry the reference's names and defaults; its training flags are accepted and ignored, as the reference's own
evaluation-only ``main_worker`` ignores them.  Nothing is parsed, created or written at import time.
"""
from __future__ import annotations

import argparse
import contextlib
import os
import subprocess
import sys
from typing import List, Optional, Sequence

VARIANT_CLASSES = {"small": "TT_vf_19lv3_imgnet_small", "xsmall": "TT_vf_19lv3_imgnet_xsmall", "full": "TT_vf_19lv3_imgnet"}
# the reference's flags that only its (absent) training loop, its log directories or its own launcher read
_IGNORED = [("--root_dir", str, "./"), ("--log_name", str, "resnet_imagenet_4w4f"), ("--pretrain_dir", str, "resnet_4w4f"),
            ("--lr", float, 0.1), ("--wd", float, 1e-4), ("--train_batch_size", int, 256), ("--max_epochs", int, 90),
            ("--Wbits", int, 32), ("--Abit_inter", int, 2), ("--world-size", int, 1), ("--rank", int, 0),
            ("--dist-url", str, "tcp://127.0.0.1:2345"), ("--dist-backend", str, "nccl"), ("--seed", int, None)]
_IGNORED_SWITCHES = ["--pretrain", "--multiprocessing-distributed"]


def add_model_flags(p: argparse.ArgumentParser, data_help: str):
    """The flags that carry the reference's names and defaults: data, loader, model geometry, device, logging."""
    ref = p.add_argument_group("flags of the reference's main.py (same names and defaults)")
    ref.add_argument("--data_dir", type=str, default="./../datasets/ILSVRC/Data/CLS-LOC/", help=data_help)
    ref.add_argument("--eval_batch_size", type=int, default=100)
    ref.add_argument("--num_workers", type=int, default=6)
    ref.add_argument("--nfilter", type=int, default=8)
    ref.add_argument("--tfilter", type=int, default=8)
    ref.add_argument("--layers", type=int, default=1)
    ref.add_argument("--groups", type=str, default="1,None,4,None")
    ref.add_argument("--gpu", type=int, default=None, help="GPU id to use (single process; default 0)")
    ref.add_argument("--log_interval", type=int, default=40, help="print running metrics every N batches (0: never)")


def add_own_flags(p: argparse.ArgumentParser):
    """Model family, checkpoint, input path, lanes and ranks: shared by ``main`` and ``predict``."""
    own = p.add_argument_group("flags of this command")
    own.add_argument("--variant", choices=sorted(VARIANT_CLASSES), default="small",
                     help="model family (the reference hard-codes small)")
    own.add_argument("--ckpt", type=str, default=None,
                     help="checkpoint with a 'model_state_dict' entry, bare or 'module.'-prefixed keys "
                          "(default ./ckpt/last.pth, the path the reference hard-codes)")
    own.add_argument("--synthetic-ckpt", action="store_true",
                     help="use synth.synth_state_dict's deterministic weights instead of a trained checkpoint; when --ckpt "
                          "names a file that does not exist yet, the synthetic checkpoint is written there first")
    own.add_argument("--input", choices=["jpeg", "jpeg-progressive", "pillow"], default="jpeg",
                     help="jpeg: files decoded on the device (progressive ones by Pillow in the workers); "
                          "jpeg-progressive: progressive files on the device too; pillow: everything decoded by Pillow "
                          "in the workers (slow; for cross-checking a folder)")
    own.add_argument("--views", choices=["flip", "five", "ten"], default=None,
                     help="multi-crop evaluation: Resize(256), then the centre crop and its flip (2 views), FiveCrop(224) or "
                          "TenCrop(224); every file is decoded once, the views are cut and forwarded on the device and their "
                          "logits averaged (default: the one centre crop).  Not with --care_from")
    own.add_argument("--inflight", type=int, default=2, help="batches in flight on separate streams / lanes")
    own.add_argument("--gpus", type=int, default=1, help="evaluate on N GPUs: starts one rank per GPU itself")
    return own


def add_topk_flags(group, default: int):
    group.add_argument("--topk", type=int, default=default, metavar="K",
                       help=f"the K best classes per image, 1 .. 32 (default {default}" + (": none)" if not default else ")"))
    group.add_argument("--classes", type=str, default=None, metavar="FILE",
                       help="class names, one per line in index order: written instead of the indices")


def add_care_flags(group):
    group.add_argument("--care_from", type=str, default=None, metavar="FILE",
                       help=".npz written by --table_usage: the entries that run read are the care set; every image is then "
                            "tested for lookups outside it, and `Care.. covered/N top1 [lo, hi] top5 [lo, hi]` brackets the "
                            "accuracy of any circuit minimised with the other entries as don't-cares")
    group.add_argument("--care_min_count", type=int, default=1, metavar="T",
                       help="keep only the entries read at least T times (default 1)")


def care_args(args) -> dict:
    """The ``evaluate`` keywords of --care_from."""
    if not args.care_from:
        return {}
    from . import report
    return dict(care=report.load_table_usage(args.care_from), care_min_count=args.care_min_count)


def check_care_flags(args):
    if args.care_min_count < 1:
        raise SystemExit("--care_min_count must be at least 1")
    if not args.care_from:
        for flag in ("care_rows", "care_summary"):
            if getattr(args, flag, None):
                raise SystemExit(f"--{flag} needs --care_from")
        if args.care_min_count != 1:
            raise SystemExit("--care_min_count needs --care_from")
    elif not os.path.isfile(args.care_from):
        raise SystemExit(f"--care_from: {args.care_from} does not exist (write it with --table_usage)")


def check_rule_flags(args):
    if not args.rule_support:
        for flag in ("rule_form", "rule_min_share"):
            if getattr(args, flag) is not None:
                raise SystemExit(f"--{flag} needs --rule_support")
    elif not (args.table_usage or args.care_from):
        raise SystemExit("--rule_support needs --table_usage or --care_from")
    if args.rule_min_share is not None and not args.rule_min_share >= 0:
        raise SystemExit("--rule_min_share must be at least 0")


def write_rule_support(args, model, usage):
    """--rule_support: the covers of every binarised block against ``usage``, pruned too with --rule_min_share."""
    from . import report, rules
    support = model.rule_support(usage, form=args.rule_form or "dnf", rounds=args.table_gates_rounds)
    pruned = None
    if args.rule_min_share is not None:
        pruned = {name: rules.prune_by_share(block, usage[name], args.rule_min_share) for name, block in support.items()}
    report.write_rule_support_csv(args.rule_support, support, pruned)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m scale_imagenet_amd.main",
        description="Evaluate <data_dir>/val (one directory per class) with a TTNet ImageNet classifier on the HIP path "
                    "and print the reference's final line, `Acc.. <top-1> <top-5>`.",
        epilog="The reference's trained checkpoint is published on a file-sharing site and cannot be fetched by this "
               "command; put it at --ckpt yourself, or try the command with --synthetic-ckpt (deterministic synthetic "
               "weights: the accuracy is then that of chance).")
    add_model_flags(p, "dataset root; <data_dir>/val is evaluated")
    add_own_flags(p)
    out = p.add_argument_group("per-image and per-class results (files written by rank 0; stdout is unchanged)")
    add_topk_flags(out, 0)
    out.add_argument("--predictions", type=str, default=None, metavar="FILE",
                     help="CSV path,target,class_1,logprob_1,.. of every image in dataset order (--topk, default 5 here)")
    out.add_argument("--per_class", type=str, default=None, metavar="FILE",
                     help="CSV class,images,hits1,hits5,predicted,acc1,acc5")
    out.add_argument("--confusion", type=str, default=None, metavar="FILE",
                     help=".npy, int64 [n_classes][n_classes] indexed [target][top-1 class]")
    out.add_argument("--table_usage", type=str, default=None, metavar="FILE",
                     help=".npz, one int64 [groups][2^n] array per Block_TT: how often the evaluation read every truth-table "
                          "entry (counted on the device; 8 bytes of device memory per table entry)")
    out.add_argument("--table_coverage", type=str, default=None, metavar="FILE",
                     help="CSV block,groups,inputs,entries,seen,share_seen,constant_groups,top1pct_share (with --table_usage)")
    out.add_argument("--table_gates", type=str, default=None, metavar="FILE",
                     help="CSV, one row per binarised Block_TT: cubes and literals of its filters' DNF / CNF covers (prime and "
                          "irredundant, minimised on the device), from the whole tables and, beside them, with the entries "
                          "this run never read as don't-cares (counts the table usage, as --table_usage does)")
    out.add_argument("--table_gates_rounds", type=int, default=0, metavar="R", choices=range(9),
                     help="reduce / expand rounds (0 .. 8) of the minimiser behind both columns of --table_gates; more rounds, "
                          "smaller covers, longer minimisation; 0: the covers it always gave")
    out.add_argument("--rule_support", type=str, default=None, metavar="FILE",
                     help="CSV, one row per binarised Block_TT: how the lookups of the table usage (this run's with --table_usage, "
                          "else the file of --care_from) fall on the cubes of its filters' covers, minimised with the entries "
                          "never read as don't-cares (--table_gates_rounds applies): cubes, literals, the share of lookups the "
                          "top 1 %% / 10 %% of cubes decide, cubes without a lookup")
    out.add_argument("--rule_form", choices=["dnf", "cnf"], default=None,
                     help="the covers --rule_support measures: of the filters (dnf, the default) or of their complements (cnf)")
    out.add_argument("--rule_min_share", type=float, default=None, metavar="S",
                     help="also prune for --rule_support: drop every cube that holds less than the share S of its group's lookups, "
                          "and report the cubes and literals kept, the lookups lost and the entries lost")
    add_care_flags(out)
    out.add_argument("--care_rows", type=str, default=None, metavar="FILE",
                     help="CSV index,covered,<one column per Block_TT>: every image's care-set misses (with --care_from)")
    out.add_argument("--care_summary", type=str, default=None, metavar="FILE",
                     help="CSV block,lookups,misses,images_with_misses and a total row (with --care_from)")
    ign = p.add_argument_group("accepted and ignored (training, logging and launcher flags of the reference)")
    for name, typ, default in _IGNORED:
        ign.add_argument(name, type=typ, default=default, help=argparse.SUPPRESS)
    for name in _IGNORED_SWITCHES:
        ign.add_argument(name, action="store_true", default=False, help=argparse.SUPPRESS)
    return p


def parse_groups(text: str) -> List[Optional[int]]:
    return [None if g.strip() == "None" else int(g) for g in text.split(",")]


def _note_ignored(args, argv: Sequence[str]):
    given = sorted({a.split("=")[0] for a in argv if a.startswith("--")} &
                   ({n for n, _, _ in _IGNORED} | set(_IGNORED_SWITCHES)))
    if given:
        print(f"note: {', '.join(given)} only matter to training or to the reference's own launcher; ignored", file=sys.stderr)


def _probe_devices() -> int:
    """Number of HIP devices, counted by a child process: the parent of the ranks must not initialise the GPU itself."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count() if torch.cuda.is_available() else 0)"],
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"could not count the HIP devices:\n{r.stderr[-2000:]}")
    return int(r.stdout.strip().splitlines()[-1])


def _check_paths(args):
    val = os.path.join(args.data_dir, "val")
    if not os.path.isdir(val):
        raise SystemExit(f"--data_dir: {val} is not a directory (expected <data_dir>/val/<class>/<image files>)")
    _check_ckpt(args)


def _check_ckpt(args):
    if not args.synthetic_ckpt and not os.path.isfile(args.ckpt or "./ckpt/last.pth"):
        raise SystemExit(f"--ckpt: {args.ckpt or './ckpt/last.pth'} does not exist.  The reference's checkpoint has to be "
                         "downloaded by hand; --synthetic-ckpt runs the command on synthetic weights instead")


def _state_dict(args, spec, rank: int):
    import torch
    if args.synthetic_ckpt:
        from . import synth
        state = {k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(spec).items()}
        if args.ckpt and rank == 0 and not os.path.exists(args.ckpt):
            tmp = f"{args.ckpt}.tmp{os.getpid()}"
            torch.save({"model_state_dict": state}, tmp)
            os.replace(tmp, args.ckpt)
        return state
    ckpt = torch.load(args.ckpt or "./ckpt/last.pth", map_location="cpu")     # main.py:220-222
    return ckpt["model_state_dict"]


class _PillowFolder:
    """``FileBytesFolder``'s samples decoded in the worker as the reference's loader does
    (``Image.open(path).convert("RGB")``): uint8 HWC images for ``collate_u8``."""

    def __init__(self, folder):
        self.samples = folder.samples

    def __len__(self) -> int:
        return len(self.samples)

    def __getitem__(self, i):
        import numpy as np
        from PIL import Image
        path, target = self.samples[i]
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB")), target


def start_rank(args, prog: str = "scale_imagenet_amd.main"):
    """Join the job, pick this rank's device: ``(rank, world, device)``."""
    import torch

    from .dist import init_from_env
    rank, world, local_rank = init_from_env("nccl")
    if world != args.gpus and world > 1:
        args.gpus = world                                 # started by torch.distributed.run: its world size holds
    if not torch.cuda.is_available():
        raise SystemExit(f"{prog} needs a HIP device (the product has no CPU path)")
    index = (args.gpu or 0) if world == 1 else local_rank % torch.cuda.device_count()
    device = torch.device("cuda", index)
    torch.cuda.set_device(device)
    return rank, world, device


def load_model(args, device, rank: int):
    from . import ttnet
    model = getattr(ttnet, VARIANT_CLASSES[args.variant])(argparse.Namespace(
        nfilter=args.nfilter, tfilter=args.tfilter, layers=args.layers, groups=parse_groups(args.groups)))
    model.load_state_dict(_state_dict(args, model.spec, rank), strict=True)
    return model.to(device).eval().reserve(max(1, args.eval_batch_size) * views_per_image(args))


def views_per_image(args) -> int:
    """How many crops --views forwards per image (1 without the flag)."""
    from ._lib import VIEW_FAMILIES
    views = getattr(args, "views", None)
    return VIEW_FAMILIES[views][1] if views else 1


def views_args(args) -> dict:
    """The ``evaluate`` keyword of --views (none without the flag: the call is what it was)."""
    if not getattr(args, "views", None):
        return {}
    if args.care_from:
        raise SystemExit("--views does not go with --care_from: the care-set misses are per forwarded crop")
    return dict(views=args.views)


def shard_loader(args, folder, rank: int, world: int):
    """This rank's ``ShardedSampler`` slice of ``folder`` (``FileBytesFolder`` / ``FileBytesList``) behind --input's collate."""
    import torch

    from . import jpeg, preprocess
    from .dist import ShardedSampler
    dataset, collate = {"jpeg": (folder, jpeg.collate_jpeg),
                        "jpeg-progressive": (folder, jpeg.collate_jpeg_progressive),
                        "pillow": (_PillowFolder(folder), preprocess.collate_u8)}[args.input]
    # the workers are fresh interpreters: this process has initialised the GPU and is not forked (launch.py)
    return torch.utils.data.DataLoader(dataset, batch_size=args.eval_batch_size, sampler=ShardedSampler(len(dataset), rank, world),
                                       num_workers=args.num_workers, collate_fn=collate, pin_memory=True,
                                       multiprocessing_context="spawn" if args.num_workers > 0 else None)


def check_topk(args, needed: bool):
    if args.topk == 0 and needed:
        args.topk = 5
    if not (0 <= args.topk <= 32):
        raise SystemExit("--topk must be in [1, 32]")


def end_ranks(world: int):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def run(args) -> int:
    """One rank (or the only process): evaluate this rank's shard, sum over the ranks, rank 0 prints the line."""
    from . import jpeg, report
    from .dist import all_gather_care, all_gather_predictions, all_reduce_counts, all_reduce_metrics, all_reduce_table_usage
    from .evaluate import evaluate

    rank, world, device = start_rank(args)
    _check_paths(args)
    model = load_model(args, device, rank)
    folder = jpeg.FileBytesFolder(os.path.join(args.data_dir, "val"))
    loader = shard_loader(args, folder, rank, world)
    extra = {}
    if args.topk or args.predictions or args.per_class or args.confusion:      # (otherwise the call is what it was)
        extra = dict(topk=args.topk, per_class=bool(args.per_class or args.confusion), confusion=bool(args.confusion))
    if args.table_usage or args.table_gates:
        extra["table_usage"] = True
    extra.update(care_args(args))
    extra.update(views_args(args))
    # a rank's own lines (running metrics, its shard's Acc..) go to stderr when there are several: stdout carries the result
    with contextlib.redirect_stdout(sys.stderr) if world > 1 else contextlib.nullcontext():
        part = evaluate(model, loader, device, log_every=args.log_interval, inflight=max(1, args.inflight), metrics="device",
                        **extra)
    res = all_reduce_metrics(part)
    if world > 1 and rank == 0:
        print("Acc..", res.top1, res.top5, flush=True)                 # main.py:284
    if args.care_from:
        care = all_gather_care(part.care)
        if world > 1 and rank == 0:
            print(care.line(), flush=True)
        if rank == 0 and args.care_rows:
            report.write_care_rows_csv(args.care_rows, care)
        if rank == 0 and args.care_summary:
            report.write_care_summary_csv(args.care_summary, care, model.care_lookups())
    if args.table_usage or args.table_gates:
        usage = all_reduce_table_usage(part.table_usage)
        if rank == 0 and args.table_usage:
            report.save_table_usage(args.table_usage, usage)
            if args.table_coverage:
                report.write_coverage_csv(args.table_coverage, usage, {name: model.get_table(name) for name in usage})
        if rank == 0 and args.table_gates:
            report.write_gates_csv(args.table_gates, model.gate_counts(rounds=args.table_gates_rounds),
                                   model.gate_counts(usage, rounds=args.table_gates_rounds),
                                   {b.name: b.fan_in_bits for b in model.spec.block_tts()})
    if rank == 0 and args.rule_support:
        write_rule_support(args, model, usage if args.table_usage else report.load_table_usage(args.care_from))
    if extra.get("topk") is not None:
        names = report.read_class_names(args.classes) if args.classes else None
        pred = all_gather_predictions(part.predictions) if args.predictions else None
        counts, confusion = all_reduce_counts(part.per_class, part.confusion) if extra["per_class"] else (None, None)
        if rank == 0:
            if args.predictions:
                report.write_predictions_csv(args.predictions, [p for p, _ in folder.samples], folder.targets, pred, names)
            if args.per_class:
                report.write_per_class_csv(args.per_class, counts, names)
            if args.confusion:
                report.write_confusion(args.confusion, confusion)
    end_ranks(world)
    return 0


def main(argv: Optional[Sequence[str]] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    check_topk(args, needed=bool(args.predictions))
    if args.table_coverage and not args.table_usage:
        raise SystemExit("--table_coverage needs --table_usage")
    if args.table_gates_rounds and not (args.table_gates or args.rule_support):
        raise SystemExit("--table_gates_rounds needs --table_gates or --rule_support")
    check_rule_flags(args)
    check_care_flags(args)
    views_args(args)
    return launch(args, argv, "scale_imagenet_amd.main", _check_paths, run)


def launch(args, argv, module: str, check_paths, run_rank) -> int:
    """Run ``run_rank(args)`` here, or -- for --gpus N from a plain command line -- start N fresh ranks of ``module``."""
    from .launch import spawn_ranks, under_launcher
    if args.gpus < 1:
        raise SystemExit("--gpus must be positive")
    if args.gpus > 1 and not under_launcher():
        # this process has not touched the GPU and does not: the ranks are fresh interpreters (launch.py)
        have = _probe_devices()
        if have < 1:
            raise SystemExit(f"--gpus {args.gpus}: no HIP device on this machine (the product has no CPU path); no rank was started")
        if have < args.gpus and os.environ.get("TTNET_DIST_BACKEND") != "gloo":
            raise SystemExit(f"--gpus {args.gpus}: only {have} HIP device(s) here (TTNET_DIST_BACKEND=gloo rehearses several "
                             "ranks on one device)")
        check_paths(args)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))       # the ranks import the same package
        path = os.pathsep.join(p for p in (root, os.environ.get("PYTHONPATH")) if p)
        return spawn_ranks(["-m", module, *argv], args.gpus, extra_env={"PYTHONPATH": path})
    if os.environ.get("RANK", "0") == "0":
        _note_ignored(args, argv)
    return run_rank(args)


if __name__ == "__main__":
    sys.exit(main())
