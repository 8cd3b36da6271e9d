"""``python -m scale_imagenet_amd.predict``: classify every image under a directory -- no ``val/``, no class directories.

The files' bytes go to the device as in ``scale_imagenet_amd.main`` (``FileBytesList`` + ``collate_jpeg``), are decoded,
resized, cropped and classified there, and ``ttnet_topk_rows`` reduces each image's logits to its K best classes on
the device: 16 * K bytes per image come back.  Rank 0 writes one CSV line per file, in sorted path order (report.py).
The model / input / lane / rank flags and the launcher are ``main``'s own.
"""
from __future__ import annotations

import argparse
import contextlib
import os
import sys
from typing import Optional, Sequence

from .main import _check_ckpt, add_care_flags, add_model_flags, add_own_flags, add_topk_flags, care_args, check_care_flags, \
    check_topk, end_ranks, launch, load_model, shard_loader, start_rank, views_args


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m scale_imagenet_amd.predict",
        description="Classify every image file under --data_dir (walked recursively, sorted) with a TTNet ImageNet "
                    "classifier on the HIP path and write path,target,class_1,logprob_1,..,class_K,logprob_K per file "
                    "(target is empty: the files carry no labels).  With --care_from a last column `covered` says, 1 or 0, "
                    "whether every table lookup of the image stayed inside the care set.")
    add_model_flags(p, "directory of image files, any layout")
    own = add_own_flags(p)
    add_topk_flags(own, 5)
    add_care_flags(own)
    own.add_argument("--out", type=str, default=None, metavar="FILE", help="the CSV (default: standard output)")
    return p


def _check_paths(args):
    if not os.path.isdir(args.data_dir):
        raise SystemExit(f"--data_dir: {args.data_dir} is not a directory")
    _check_ckpt(args)


def run(args) -> int:
    """One rank (or the only process): classify this rank's shard, join the shards, rank 0 writes the file."""
    from . import jpeg, report
    from .dist import all_gather_care, all_gather_predictions
    from .evaluate import evaluate

    rank, world, device = start_rank(args, "scale_imagenet_amd.predict")
    _check_paths(args)
    model = load_model(args, device, rank)
    files = jpeg.FileBytesList(args.data_dir)
    loader = shard_loader(args, files, rank, world)
    with contextlib.redirect_stdout(sys.stderr):          # stdout carries the CSV (or nothing)
        part = evaluate(model, ((inputs, None) for inputs, _ in loader), device, inflight=max(1, args.inflight), topk=args.topk,
                        **care_args(args), **views_args(args))
    pred = all_gather_predictions(part.predictions)
    covered = all_gather_care(part.care).covered if args.care_from else None
    if rank == 0:
        names = report.read_class_names(args.classes) if args.classes else None
        report.write_predictions_csv(args.out, files.paths, None, pred, names, covered)
    end_ranks(world)
    return 0


def main(argv: Optional[Sequence[str]] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    check_topk(args, needed=True)
    check_care_flags(args)
    views_args(args)
    return launch(args, argv, "scale_imagenet_amd.predict", _check_paths, run)


if __name__ == "__main__":
    sys.exit(main())
