"""CIFAR-10 for ``TT_FHE_XSMALL_vAlexnet``: the dataset's files, batches that live on the device, and the command
``python -m scale_imagenet_amd.cifar``.

The reference feeds this model ``cifar_transform(False)`` (utils/preprocess.py:82-87): ``ToTensor`` and
``Normalize(CIFAR_MEAN, CIFAR_STD)``, nothing else -- no decoding, resizing or cropping.  So the images stay what the
dataset holds, bytes: ``read_cifar10`` transposes the files' planar CHW records to HWC once on the host,
``device_batches`` uploads the whole split once (30 MB for the test set) and hands out slices of it, and
``model.forward_u8`` normalises inside the stem kernel (include/ttnet.h: ttnet_forward_u8).  ``evaluate`` sends uint8
tensors there by itself.  ``--certify EPS[,EPS...]`` then certifies the labels against perturbations of up to EPS byte levels
over the same device-resident bytes (``scale_imagenet_amd.certify``) and prints the verified accuracy per eps; with
``--attack`` a search for uint8 counter-examples follows (``scale_imagenet_amd.attack``) and one ``Robust..`` line per eps
brackets the robust accuracy from both sides.  ``--certify_patch HxW[,..]`` sweeps a patch over every image, and with
``--attack_patch`` a search for a falsifying fill per position follows: one ``PatchRobust..`` line per size.

Both published layouts are read: ``cifar-10-batches-py`` (pickles ``test_batch`` / ``data_batch_1..5``, ``batches.meta``)
and ``cifar-10-batches-bin`` (``*.bin`` records of 1 label byte + 3072 planar bytes, ``batches.meta.txt``).  The pickles go
through a restricted unpickler: a dataset file cannot name a callable other than numpy's array reconstruction.
Nothing is parsed, created or written at import time.
"""
from __future__ import annotations

import argparse
import io
import os
import pickle
import sys
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

# cifar_transform, utils/preprocess.py:82-87 (the defaults of a vAlexnet plan, include/ttnet.h)
CIFAR_MEAN = (0.4914, 0.4822, 0.4465)
CIFAR_STD = (0.2023, 0.1994, 0.2010)
N_CLASSES = 10
RECORD_BYTES = 1 + 3072                       # cifar-10-batches-bin: label, then 1024 R, 1024 G, 1024 B bytes
LAYOUT_DIRS = ("cifar-10-batches-py", "cifar-10-batches-bin")
SPLIT_FILES = {"test": ["test_batch"], "train": [f"data_batch_{i}" for i in range(1, 6)]}


def _numpy_globals():
    """The globals a pickled numpy array names: ``_reconstruct`` (under numpy.core or numpy._core, by the numpy that wrote
    the file), ``ndarray``, ``dtype``, and ``_codecs.encode``, through which Python 3 writes an array's bytes at pickle
    protocol 2 (it turns a str into bytes and does nothing else).  Resolved here, never imported by name from the file."""
    import _codecs
    reconstruct = np.zeros(0, dtype=np.uint8).__reduce__()[0]
    return {("numpy.core.multiarray", "_reconstruct"): reconstruct, ("numpy._core.multiarray", "_reconstruct"): reconstruct,
            ("numpy", "ndarray"): np.ndarray, ("numpy", "dtype"): np.dtype, ("_codecs", "encode"): _codecs.encode}


class RefusedGlobal(pickle.UnpicklingError):
    """A dataset pickle named a global that a CIFAR file has no use for."""


class _ArrayUnpickler(pickle.Unpickler):
    """Unpickles containers, numbers, strings and numpy arrays; any other global is refused."""

    def __init__(self, f, name: str):
        super().__init__(f, encoding="bytes")
        self._name = name
        self._allowed = _numpy_globals()

    def find_class(self, module, name):
        try:
            return self._allowed[(module, name)]
        except KeyError:
            raise RefusedGlobal(f"{self._name}: the pickle names the global {module}.{name}; a CIFAR file holds only lists, "
                                "numbers, strings and numpy arrays, so it is refused") from None


def load_pickle(path: str):
    """A dataset pickle through the restricted unpickler (keys come back as bytes, as the files have them)."""
    with open(path, "rb") as f:
        data = f.read()
    try:
        return _ArrayUnpickler(io.BytesIO(data), path).load()
    except RefusedGlobal:
        raise
    except Exception as e:                                  # (a truncated or foreign file)
        raise ValueError(f"{path}: not a readable pickle ({type(e).__name__}: {e})") from e


def _dataset_dir(path: str, names: Sequence[str]) -> str:
    """``path`` itself or the one published directory under it that holds any of ``names``."""
    tried = [path] + [os.path.join(path, d) for d in LAYOUT_DIRS]
    for d in tried:
        if any(os.path.isfile(os.path.join(d, n)) for n in names):
            return d
    raise FileNotFoundError(f"{path}: none of {', '.join(names)} here or under {' / '.join(LAYOUT_DIRS)}")


def _check_labels(labels: np.ndarray, n: int, file: str) -> np.ndarray:
    if labels.shape != (n,):
        raise ValueError(f"{file}: {labels.size} labels for {n} images")
    if n and (labels.min() < 0 or labels.max() >= N_CLASSES):
        bad = int(labels[(labels < 0) | (labels >= N_CLASSES)][0])
        raise ValueError(f"{file}: label {bad} is outside [0, {N_CLASSES - 1}]")
    return labels.astype(np.int64)


def _read_py(file: str) -> Tuple[np.ndarray, np.ndarray]:
    d = load_pickle(file)
    if not isinstance(d, dict) or b"data" not in d or b"labels" not in d:
        raise ValueError(f"{file}: expected a dict with b'data' and b'labels'")
    data = d[b"data"]
    if not isinstance(data, np.ndarray) or data.dtype != np.uint8 or data.ndim != 2 or data.shape[1] != 3072:
        what = f"{data.dtype} {tuple(data.shape)}" if isinstance(data, np.ndarray) else type(data).__name__
        raise ValueError(f"{file}: b'data' must be uint8 [N, 3072], got {what}")
    return data, _check_labels(np.asarray(d[b"labels"], dtype=np.int64).reshape(-1), data.shape[0], file)


def _read_bin(file: str) -> Tuple[np.ndarray, np.ndarray]:
    raw = np.fromfile(file, dtype=np.uint8)
    if raw.size % RECORD_BYTES:
        raise ValueError(f"{file}: {raw.size} bytes is not a whole number of {RECORD_BYTES}-byte records "
                         f"({raw.size % RECORD_BYTES} left over)")
    rec = raw.reshape(-1, RECORD_BYTES)
    return rec[:, 1:], _check_labels(rec[:, 0].astype(np.int64), rec.shape[0], file)


def read_cifar10(path: str, split: str = "test") -> Tuple[np.ndarray, np.ndarray]:
    """``(uint8 [N, 32, 32, 3], int64 [N])`` of ``split`` ("test" or "train") from ``path``: a ``cifar-10-batches-py`` or
    ``cifar-10-batches-bin`` directory, or the directory that holds one.  The train split is ``data_batch_1``, ``_2``, ..
    in order, as many as are there without a gap.  Pixel ``[r, q, c]`` is byte ``c * 1024 + r * 32 + q`` of its record."""
    if split not in SPLIT_FILES:
        raise ValueError(f"split must be \"test\" or \"train\", got {split!r}")
    stems = SPLIT_FILES[split]
    d = _dataset_dir(path, [s + ext for s in stems for ext in ("", ".bin")])
    binary = not os.path.isfile(os.path.join(d, stems[0]))
    files = [os.path.join(d, s + (".bin" if binary else "")) for s in stems]
    if not os.path.isfile(files[0]):
        raise FileNotFoundError(f"{files[0]}: the {split} split starts with this file")
    present = [os.path.isfile(f) for f in files]
    count = present.index(False) if False in present else len(files)
    if any(present[count:]):
        raise FileNotFoundError(f"{files[count]}: missing, but a later batch of the {split} split is there")
    parts = [(_read_bin if binary else _read_py)(f) for f in files[:count]]
    planar = np.concatenate([p[0] for p in parts])
    images = np.ascontiguousarray(planar.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))     # CHW -> HWC, once
    return images, np.concatenate([p[1] for p in parts])


def read_label_names(path: str) -> List[str]:
    """The ten class names from ``batches.meta`` (pickle, ``b'label_names'``) or ``batches.meta.txt`` (one per line)."""
    d = _dataset_dir(path, ["batches.meta", "batches.meta.txt"])
    file = os.path.join(d, "batches.meta")
    if os.path.isfile(file):
        meta = load_pickle(file)
        if not isinstance(meta, dict) or b"label_names" not in meta:
            raise ValueError(f"{file}: expected a dict with b'label_names'")
        names = [n.decode("utf-8") if isinstance(n, bytes) else str(n) for n in meta[b"label_names"]]
    else:
        from .report import read_class_names
        file += ".txt"
        names = read_class_names(file)
    if len(names) != N_CLASSES:
        raise ValueError(f"{file}: {len(names)} class names, expected {N_CLASSES}")
    return names


def device_batches(images, targets, batch_size: int, device) -> Iterator[Tuple["torch.Tensor", "torch.Tensor"]]:
    """Upload ``images`` (uint8 ``[N, 32, 32, 3]``) and ``targets`` (int64 ``[N]``) to ``device`` once, then yield
    ``(images[a:b], targets[a:b])`` in order, ``batch_size`` at a time (the last pair may be shorter): the batches
    ``evaluate`` sends to ``model.forward_u8``.  No loader, no worker, no host copy per batch."""
    import torch
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    x = torch.as_tensor(images)
    t = torch.as_tensor(targets)
    if x.dtype != torch.uint8 or x.dim() != 4 or tuple(x.shape[1:]) != (32, 32, 3):
        raise ValueError(f"expected uint8 images [N, 32, 32, 3], got {x.dtype} {tuple(x.shape)}")
    if t.dtype != torch.int64 or tuple(t.shape) != (x.shape[0],):
        raise ValueError(f"expected int64 targets [{x.shape[0]}], got {t.dtype} {tuple(t.shape)}")
    x, t = x.contiguous().to(device), t.to(device)
    for a in range(0, x.shape[0], batch_size):
        yield x[a:a + batch_size], t[a:a + batch_size]


# ---- python -m scale_imagenet_amd.cifar ------------------------------------------------------------------------------

def build_parser() -> argparse.ArgumentParser:
    from .main import add_topk_flags
    p = argparse.ArgumentParser(
        prog="python -m scale_imagenet_amd.cifar",
        description="Evaluate a CIFAR-10 split with TT_FHE_XSMALL_vAlexnet on the HIP path and print the reference's final "
                    "line, `Acc.. <top-1> <top-5>`.  The split is uploaded once as bytes and normalised inside the stem kernel.",
        epilog="No trained checkpoint is published with the reference for this model; --synthetic-ckpt runs the command on "
               "deterministic synthetic weights (the accuracy is then that of chance).")
    p.add_argument("--data_dir", type=str, default="./../datasets/", help="cifar-10-batches-py or cifar-10-batches-bin, or the "
                   "directory that holds one of them")
    p.add_argument("--split", choices=sorted(SPLIT_FILES), default="test")
    p.add_argument("--ckpt", type=str, default=None,
                   help="checkpoint with a 'model_state_dict' entry, bare or 'module.'-prefixed keys (default ./ckpt/last.pth)")
    p.add_argument("--synthetic-ckpt", action="store_true",
                   help="use synth.synth_state_dict's deterministic weights instead of a trained checkpoint; when --ckpt names "
                        "a file that does not exist yet, the synthetic checkpoint is written there first")
    p.add_argument("--eval_batch_size", type=int, default=256)
    p.add_argument("--inflight", type=int, default=2, help="batches in flight on separate streams / lanes")
    p.add_argument("--gpu", type=int, default=None, help="GPU id to use (default 0)")
    out = p.add_argument_group("per-image and per-class results (stdout is unchanged)")
    add_topk_flags(out, 0)
    out.add_argument("--predictions", type=str, default=None, metavar="FILE",
                     help="CSV path,target,class_1,logprob_1,.. of every image in dataset order, path = <split>/<index> "
                          "(--topk, default 5 here)")
    out.add_argument("--per_class", type=str, default=None, metavar="FILE", help="CSV class,images,hits1,hits5,predicted,acc1,acc5")
    out.add_argument("--confusion", type=str, default=None, metavar="FILE",
                     help=".npy, int64 [10][10] indexed [target][top-1 class]")
    cert = p.add_argument_group("certified L-infinity robustness of the labels (one more stdout line per eps, after `Acc..`)")
    cert.add_argument("--certify", type=str, default=None, metavar="EPS[,EPS...]",
                      help="certify every image's label against perturbations of up to EPS byte levels (2 is 2/255) and print "
                           "`Verified.. eps=E certified/N pct (interval a, enumeration b; unknown stem bits median u max v)`: "
                           "the verified accuracy.  Sound, not complete (scale_imagenet_amd.certify)")
    cert.add_argument("--certify_enum", type=int, default=10, metavar="K",
                      help="settle images with up to K unknown stem bits by enumeration (0..12, 0: interval bound only)")
    cert.add_argument("--certify_min_margin", type=float, default=1e-6, metavar="M", help="certified means lower bound > M")
    cert.add_argument("--certify_rows", type=str, default=None, metavar="FILE",
                      help="CSV eps,index,class,stage,certified,lb,lb_interval,worst,unknown_stem,unknown_feat of every image")
    pat = p.add_argument_group("certified patch robustness of the labels (one more stdout line per patch size, after every line above)")
    pat.add_argument("--certify_patch", type=str, default=None, metavar="HxW[,HxW...]",
                     help="certify every image's label against a patch of H x W pixels (1..8 each) at every position and print "
                          "`Patch.. size=HxW amp=A stride=S certified/N pct (positions p/P certified: interval a, enumeration b; "
                          "unknown stem bits median u max v)`; --certify_enum and --certify_min_margin apply")
    pat.add_argument("--patch_stride", type=int, default=1, metavar="S",
                     help="positions every S pixels (1..32); above 1 the line says `sampled`: only stride 1 covers every placement")
    pat.add_argument("--patch_amp", type=int, default=255, metavar="A", help="the patch's bytes move by up to A levels (1..255; 255: any value)")
    pat.add_argument("--patch_map", type=str, default=None, metavar="FILE",
                     help=".npz: per size lb_HxW, stage_HxW, worst_HxW, unknown_stem_HxW, each [N][Py][Px]")
    pat.add_argument("--patch_rows", type=str, default=None, metavar="FILE",
                     help="CSV size,amp,stride,index,class,patch_certified,certified,positions,interval,enumeration,lb_min,pos_min,worst")
    pat.add_argument("--attack_patch", action="store_true",
                     help="after each `Patch..` line, search every position for a uint8 fill of the patch on which the image loses its label "
                          "and print `PatchRobust.. certified a/N <= robust <= b/N`; a witness counts once forward_u8 has judged it "
                          "(scale_imagenet_amd.attack)")
    pat.add_argument("--attack_patch_rounds", type=int, default=2, metavar="R", help="rounds of the patch search (1..4)")
    pat.add_argument("--attack_patch_confirm", choices=("all", "best"), default="all",
                     help="forward every predicted witness, or only each image's most promising position (enough for the bracket)")
    pat.add_argument("--patch_witnesses", type=str, default=None, metavar="FILE",
                     help=".npz of the falsified positions per size: tasks_HxW, fills_HxW, margin_HxW, m_pred_HxW, geometry_HxW")
    att = p.add_argument_group("falsified robustness (with --certify: one more stdout line per eps, after its `Verified..`)")
    att.add_argument("--attack", action="store_true",
                     help="search the box of floor(EPS) byte levels for a uint8 image that loses the label and print `Robust.. eps=E "
                          "certified a/N <= robust <= b/N (falsified f: wrong at x0 w, by search s; open o)`.  A search, not a "
                          "decision: an open image stays open.  An EPS below 1 is skipped (scale_imagenet_amd.attack)")
    att.add_argument("--attack_rounds", type=int, default=3, metavar="R", help="rounds of the search (0..8; 0: only the images wrong at x0)")
    att.add_argument("--attack_rows", type=str, default=None, metavar="FILE",
                     help="CSV eps,index,class,status,falsified,margin0,best,worst,round,changed,linf,tried of every image")
    att.add_argument("--attack_witnesses", type=str, default=None, metavar="FILE",
                     help=".npz: per searched eps `eps_<E>` uint8 [N][32][32][3], the image of the smallest margin found (a "
                          "counter-example where the record says falsified), and `status_<E>`")
    return p


def certify_eps_list(text: Optional[str]) -> List[float]:
    """The eps values of ``--certify``: comma-separated, finite, not negative."""
    if not text:
        return []
    try:
        eps = [float(t) for t in text.split(",")]
    except ValueError:
        raise SystemExit(f"--certify: {text!r} is not a comma-separated list of numbers") from None
    if any(not (np.isfinite(e) and e >= 0) for e in eps):
        raise SystemExit("--certify: every eps must be finite and >= 0")
    return eps


def certify_patch_list(text: Optional[str]) -> List[tuple]:
    """The sizes of ``--certify_patch``: comma-separated ``HxW``, each side 1..8."""
    if not text:
        return []
    try:
        sizes = [tuple(int(v) for v in t.split("x")) for t in text.split(",")]
    except ValueError:
        raise SystemExit(f"--certify_patch: {text!r} is not a comma-separated list of HxW") from None
    if any(len(p) != 2 or not all(1 <= v <= 8 for v in p) for p in sizes):
        raise SystemExit("--certify_patch: every size is HxW with H and W in 1..8")
    return sizes


def _class_names(args) -> Optional[List[str]]:
    """--classes FILE, else the dataset's own batches.meta when it is there."""
    from . import report
    if args.classes:
        return report.read_class_names(args.classes)
    try:
        return read_label_names(args.data_dir)
    except FileNotFoundError:
        return None


def run(args) -> int:
    import torch

    from . import report, ttnet
    from .evaluate import evaluate
    from .main import _check_ckpt, _state_dict
    if not os.path.isdir(args.data_dir):
        raise SystemExit(f"--data_dir: {args.data_dir} is not a directory")
    _check_ckpt(args)
    if args.eval_batch_size < 1:
        raise SystemExit("--eval_batch_size must be positive")
    images, targets = read_cifar10(args.data_dir, args.split)
    if not torch.cuda.is_available():
        raise SystemExit("scale_imagenet_amd.cifar needs a HIP device (the product has no CPU path)")
    device = torch.device("cuda", args.gpu or 0)
    torch.cuda.set_device(device)
    model = ttnet.TT_FHE_XSMALL_vAlexnet(argparse.Namespace(nfilter=8, tfilter=8, layers=1, groups=[1, None, 4, None]))
    model.load_state_dict(_state_dict(args, model.spec, 0), strict=True)
    model = model.to(device).eval().reserve(args.eval_batch_size)
    extra = {}
    if args.topk or args.predictions or args.per_class or args.confusion:
        extra = dict(topk=args.topk, per_class=bool(args.per_class or args.confusion), confusion=bool(args.confusion))
    eps_list = certify_eps_list(args.certify)
    batches = device_batches(images, targets, args.eval_batch_size, device)
    patches = certify_patch_list(args.certify_patch)
    if eps_list or patches:
        batches = list(batches)                                 # one upload: the certificate reads the bytes the evaluation read
    res = evaluate(model, batches, device, inflight=max(1, args.inflight),
                   metrics="device", **extra)                   # prints `Acc.. top1 top5` (main.py:284)
    if extra:
        names = _class_names(args)
        if args.predictions:
            report.write_predictions_csv(args.predictions, [f"{args.split}/{i}" for i in range(len(targets))], targets.tolist(),
                                         res.predictions, names)
        if args.per_class:
            report.write_per_class_csv(args.per_class, res.per_class, names)
        if args.confusion:
            report.write_confusion(args.confusion, res.confusion)
    if eps_list:
        from . import certify
        sums = certify.certify_batches(model, batches, eps_list, args.certify_enum, args.certify_min_margin)
        searched = {}
        if args.attack:                                         # the same min_margin for both sides of the bracket
            from . import attack
            todo = [e for e in eps_list if e >= 1]
            found = attack.attack_batches(model, batches, todo, args.attack_rounds, args.certify_min_margin,
                                          keep_witnesses=bool(args.attack_witnesses))
            searched = dict(zip(todo, found))
        for s in sums:
            print(certify.verified_line(s))
            if not args.attack:
                continue
            if s["eps"] not in searched:
                print(f"Robust.. eps={s['eps']:g} not searched: the search moves whole byte levels and floor(eps) is 0")
                continue
            a = searched[s["eps"]]
            note = "" if a["levels"] == s["eps"] else f" [searched at floor(eps) = {a['levels']} byte levels]"
            print(attack.robust_line(s["eps"], s["rows"], a["rows"]) + note)
        if args.certify_rows:
            certify.write_rows_csv(args.certify_rows, sums, targets.tolist())
        if args.attack_rows:
            attack.write_rows_csv(args.attack_rows, list(searched.values()), targets.tolist())
        if args.attack_witnesses:
            from .report import replacing
            arrays = {}
            for e, a in searched.items():
                arrays[f"eps_{e:g}"] = a["witnesses"]
                arrays[f"status_{e:g}"] = a["rows"]["status"]
            with replacing(args.attack_witnesses, "wb") as f:
                np.savez(f, **arrays)
    if patches:
        from . import certify
        psums = certify.certify_patch_batches(model, batches, patches, args.patch_stride, args.patch_amp, args.certify_enum,
                                              args.certify_min_margin)
        found = []
        if args.attack_patch:                                   # the same min_margin for both sides of the bracket
            from . import attack
            found = attack.attack_patch_batches(model, batches, patches, args.patch_stride, args.patch_amp, args.attack_patch_rounds,
                                                args.certify_min_margin, args.attack_patch_confirm)
        for i, s in enumerate(psums):
            print(certify.patch_line(s))
            if found:
                print(attack.patch_robust_line(s, found[i]))
        if args.patch_witnesses:
            attack.write_patch_witnesses_npz(args.patch_witnesses, found)
        if args.patch_rows:
            certify.write_patch_rows_csv(args.patch_rows, psums, targets.tolist())
        if args.patch_map:
            certify.write_patch_map_npz(args.patch_map, psums)
    return 0


def main(argv: Optional[Sequence[str]] = None) -> int:
    from .main import check_topk
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    check_topk(args, needed=bool(args.predictions))
    if args.topk > N_CLASSES:
        raise SystemExit(f"--topk must be in [1, {N_CLASSES}]")
    certify_eps_list(args.certify)
    if not 0 <= args.certify_enum <= 12:
        raise SystemExit("--certify_enum must be in [0, 12]")
    if args.certify_rows and not args.certify:
        raise SystemExit("--certify_rows needs --certify")
    if args.attack and not args.certify:
        raise SystemExit("--attack needs --certify EPS[,EPS...]")
    certify_patch_list(args.certify_patch)
    if not 1 <= args.patch_stride <= 32:
        raise SystemExit("--patch_stride must be in [1, 32]")
    if not 1 <= args.patch_amp <= 255:
        raise SystemExit("--patch_amp must be in [1, 255]")
    if (args.patch_map or args.patch_rows) and not args.certify_patch:
        raise SystemExit("--patch_map and --patch_rows need --certify_patch HxW[,HxW...]")
    if args.attack_patch and not args.certify_patch:
        raise SystemExit("--attack_patch needs --certify_patch HxW[,HxW...]")
    if args.patch_witnesses and not args.attack_patch:
        raise SystemExit("--patch_witnesses needs --attack_patch")
    if not 1 <= args.attack_patch_rounds <= 4:
        raise SystemExit("--attack_patch_rounds must be in [1, 4]")
    if (args.attack_rows or args.attack_witnesses) and not args.attack:
        raise SystemExit("--attack_rows and --attack_witnesses need --attack")
    if not 0 <= args.attack_rounds <= 8:
        raise SystemExit("--attack_rounds must be in [0, 8]")
    if args.attack and any(e >= 65 for e in certify_eps_list(args.certify)):
        raise SystemExit("--attack: eps must be below 65 byte levels")
    return run(args)


if __name__ == "__main__":
    sys.exit(main())
