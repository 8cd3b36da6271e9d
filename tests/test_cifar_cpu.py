"""CPU: the CIFAR-10 reader (both published layouts, restricted unpickler, malformed files), the parser of
``python -m scale_imagenet_amd.cifar`` and ``device_batches`` on the CPU device."""
import collections
import os
import pickle

import numpy as np
import pytest
import torch

from scale_imagenet_amd import cifar
from scale_imagenet_amd import main as M

COUNTS = (7, 5)                     # records of data_batch_1, data_batch_2


def _records(seed=11):
    """Seeded planar records [12, 3072] and labels, as the files hold them."""
    rng = np.random.default_rng(seed)
    n = sum(COUNTS)
    return rng.integers(0, 256, size=(n, 3072), dtype=np.uint8), rng.integers(0, 10, size=n, dtype=np.int64)


def _write_py(d, data, labels, names=("data_batch_1", "data_batch_2")):
    """torchvision's layout: pickled dicts with bytes keys, b'data' a uint8 array, b'labels' a list."""
    os.makedirs(d, exist_ok=True)
    a = 0
    for name, cnt in zip(names, COUNTS):
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump({b"batch_label": name.encode(), b"labels": labels[a:a + cnt].tolist(), b"data": data[a:a + cnt].copy(),
                         b"filenames": [b"img_%d.png" % i for i in range(a, a + cnt)]}, f, protocol=2)
        a += cnt


def _write_bin(d, data, labels, names=("data_batch_1.bin", "data_batch_2.bin")):
    os.makedirs(d, exist_ok=True)
    a = 0
    for name, cnt in zip(names, COUNTS):
        rec = np.concatenate([labels[a:a + cnt, None].astype(np.uint8), data[a:a + cnt]], axis=1)
        assert rec.shape == (cnt, cifar.RECORD_BYTES)
        rec.tofile(os.path.join(d, name))
        a += cnt


def test_both_layouts_give_the_same_hwc_bytes(tmp_path):
    data, labels = _records()
    py, bn = str(tmp_path / "cifar-10-batches-py"), str(tmp_path / "b" / "cifar-10-batches-bin")
    _write_py(py, data, labels)
    _write_bin(bn, data, labels)
    got = [cifar.read_cifar10(py, "train"), cifar.read_cifar10(bn, "train"),
           cifar.read_cifar10(str(tmp_path), "train"),             # the directory that holds the layout's directory
           cifar.read_cifar10(str(tmp_path / "b"), "train")]
    for x, t in got:
        assert x.dtype == np.uint8 and x.shape == (12, 32, 32, 3) and x.flags.c_contiguous
        assert t.dtype == np.int64 and np.array_equal(t, labels)
        assert np.array_equal(x, got[0][0])
    x = got[0][0]
    rng = np.random.default_rng(3)
    for i, r, q, c in rng.integers(0, [12, 32, 32, 3], size=(200, 4)):
        assert x[i, r, q, c] == data[i, c * 1024 + r * 32 + q]
    assert np.array_equal(x, data.reshape(12, 3, 32, 32).transpose(0, 2, 3, 1))
    # the test split is its own file; a split whose first file is missing says which
    with pytest.raises(FileNotFoundError, match="test_batch"):
        cifar.read_cifar10(py, "test")
    _write_py(py, data, labels, names=("test_batch", "unused"))
    xt, tt = cifar.read_cifar10(py, "test")
    assert np.array_equal(xt, x[:7]) and np.array_equal(tt, labels[:7])
    with pytest.raises(ValueError, match="split"):
        cifar.read_cifar10(py, "val")


def test_pickle_protocols_and_numpy_module_paths(tmp_path):
    """Whatever protocol wrote the file, and under either module path numpy has pickled ``_reconstruct`` with."""
    data, labels = _records(5)
    for proto in (2, 3, 4):
        f = tmp_path / f"p{proto}"
        with open(f, "wb") as fh:
            pickle.dump({b"data": data, b"labels": labels.tolist()}, fh, protocol=proto)
        d = cifar.load_pickle(str(f))
        assert np.array_equal(d[b"data"], data) and d[b"labels"] == labels.tolist()
        raw = f.read_bytes()
        old, new = b"numpy._core.multiarray", b"numpy.core.multiarray"
        if proto == 2 and (old in raw) != (new in raw):              # text opcodes: the other spelling is a plain rewrite
            other = raw.replace(old, new) if old in raw else raw.replace(new, old)
            (tmp_path / "other").write_bytes(other)
            assert np.array_equal(cifar.load_pickle(str(tmp_path / "other"))[b"data"], data)


def test_restricted_unpickler_refuses_other_globals(tmp_path):
    f = tmp_path / "test_batch"
    with open(f, "wb") as fh:
        pickle.dump({b"data": collections.OrderedDict(a=1), b"labels": [0]}, fh, protocol=2)
    with pytest.raises(pickle.UnpicklingError, match=r"test_batch.*collections\.OrderedDict"):
        cifar.load_pickle(str(f))
    with pytest.raises(pickle.UnpicklingError, match="OrderedDict"):
        cifar.read_cifar10(str(tmp_path), "test")
    # numpy globals other than the array reconstruction are not admitted either
    with open(f, "wb") as fh:
        pickle.dump({b"data": np.float64(1.0)}, fh, protocol=2)
    with pytest.raises(pickle.UnpicklingError, match="scalar"):
        cifar.load_pickle(str(f))


def test_malformed_files_name_the_file(tmp_path):
    data, labels = _records()
    bn = tmp_path / "cifar-10-batches-bin"
    _write_bin(str(bn), data, labels, names=("test_batch.bin", "x.bin"))
    good = (bn / "test_batch.bin").read_bytes()
    (bn / "test_batch.bin").write_bytes(good[:-100])                          # truncated
    with pytest.raises(ValueError, match=r"test_batch\.bin.*3073"):
        cifar.read_cifar10(str(bn), "test")
    bad = bytearray(good)
    bad[3 * cifar.RECORD_BYTES] = 10                                          # label of record 3
    (bn / "test_batch.bin").write_bytes(bytes(bad))
    with pytest.raises(ValueError, match=r"test_batch\.bin.*label 10"):
        cifar.read_cifar10(str(bn), "test")
    py = tmp_path / "cifar-10-batches-py"
    py.mkdir()
    cases = {"shape": {b"data": data[:7, :3071].copy(), b"labels": labels[:7].tolist()},
             "dtype": {b"data": data[:7].astype(np.int16), b"labels": labels[:7].tolist()},
             "label 10": {b"data": data[:7].copy(), b"labels": [0, 1, 2, 10, 4, 5, 6]},
             "labels for": {b"data": data[:7].copy(), b"labels": labels[:6].tolist()},
             "b'labels'": {b"data": data[:7].copy()}}
    for what, d in cases.items():
        with open(py / "test_batch", "wb") as fh:
            pickle.dump(d, fh, protocol=2)
        with pytest.raises(ValueError, match="test_batch") as e:
            cifar.read_cifar10(str(py), "test")
        assert what in ("shape", "dtype") or what in str(e.value), str(e.value)
        if what in ("shape", "dtype"):
            assert "3072" in str(e.value)
    (py / "test_batch").write_bytes(b"not a pickle")
    with pytest.raises(ValueError, match="test_batch"):
        cifar.read_cifar10(str(py), "test")
    with pytest.raises(FileNotFoundError):
        cifar.read_cifar10(str(tmp_path / "nowhere"), "test")
    # a gap in the train split
    _write_py(str(py), data, labels, names=("data_batch_1", "data_batch_3"))
    with pytest.raises(FileNotFoundError, match="data_batch_2"):
        cifar.read_cifar10(str(py), "train")


def test_label_names_both_forms(tmp_path):
    names = ["airplane", "automobile", "bird", "cat", "deer", "dog", "frog", "horse", "ship", "truck"]
    py, bn = tmp_path / "cifar-10-batches-py", tmp_path / "cifar-10-batches-bin"
    py.mkdir()
    bn.mkdir()
    with open(py / "batches.meta", "wb") as fh:
        pickle.dump({b"num_cases_per_batch": 10000, b"label_names": [n.encode() for n in names], b"num_vis": 3072}, fh, protocol=2)
    (bn / "batches.meta.txt").write_text("\n".join(names) + "\n\n")
    assert cifar.read_label_names(str(py)) == names
    assert cifar.read_label_names(str(bn)) == names
    assert cifar.read_label_names(str(tmp_path)) == names
    (bn / "batches.meta.txt").write_text("\n".join(names[:9]) + "\n")
    with pytest.raises(ValueError, match=r"batches\.meta\.txt.*9 class names"):
        cifar.read_label_names(str(bn))


def test_parser_defaults_and_checkpoint_flags(tmp_path):
    a = cifar.build_parser().parse_args([])
    assert (a.eval_batch_size, a.split, a.topk, a.gpu, a.ckpt, a.synthetic_ckpt) == (256, "test", 0, None, None, False)
    assert (a.predictions, a.per_class, a.confusion, a.classes) == (None, None, None, None)
    assert a.inflight == M.build_parser().parse_args([]).inflight
    assert not hasattr(a, "gpus") and not hasattr(a, "variant") and not hasattr(a, "views")
    a = cifar.build_parser().parse_args(["--data_dir", "d", "--synthetic-ckpt", "--ckpt", "c.pth", "--split", "train", "--topk", "3",
                                         "--eval_batch_size", "128", "--inflight", "1", "--gpu", "2", "--predictions", "p.csv",
                                         "--per_class", "c.csv", "--confusion", "m.npy", "--classes", "names.txt"])
    assert (a.data_dir, a.synthetic_ckpt, a.ckpt, a.split, a.topk, a.eval_batch_size, a.inflight, a.gpu) == \
        ("d", True, "c.pth", "train", 3, 128, 1, 2)
    assert (a.predictions, a.per_class, a.confusion, a.classes) == ("p.csv", "c.csv", "m.npy", "names.txt")
    with pytest.raises(SystemExit):
        cifar.build_parser().parse_args(["--split", "val"])
    # --ckpt / --synthetic-ckpt as in main: a missing checkpoint is refused before any device work, unless synthetic
    (tmp_path / "cifar-10-batches-bin").mkdir()
    with pytest.raises(SystemExit, match="does not exist"):
        cifar.main(["--data_dir", str(tmp_path), "--ckpt", str(tmp_path / "none.pth")])
    with pytest.raises(SystemExit, match="topk"):
        cifar.main(["--data_dir", str(tmp_path), "--synthetic-ckpt", "--topk", "11"])
    with pytest.raises(SystemExit, match="not a directory"):
        cifar.main(["--data_dir", str(tmp_path / "nowhere"), "--synthetic-ckpt"])
    # main's own model families are what they were
    variant = next(x for x in M.build_parser()._actions if x.dest == "variant")
    assert sorted(variant.choices) == ["full", "small", "xsmall"] and sorted(M.VARIANT_CLASSES) == ["full", "small", "xsmall"]


def test_synthetic_checkpoint_is_written_and_read_back(tmp_path):
    """main's checkpoint helpers on the vAlexnet layout: --synthetic-ckpt --ckpt F writes F, --ckpt F reads the same tensors."""
    from argparse import Namespace
    from scale_imagenet_amd.spec import VAlexSpec
    ck = str(tmp_path / "va.pth")
    st = M._state_dict(Namespace(synthetic_ckpt=True, ckpt=ck), VAlexSpec(), 0)
    assert os.path.isfile(ck) and len(st) == 57
    back = M._state_dict(Namespace(synthetic_ckpt=False, ckpt=ck), VAlexSpec(), 0)
    assert list(back) == list(st) and all(torch.equal(back[k], st[k]) for k in st)


def test_device_batches_on_cpu():
    rng = np.random.default_rng(2)
    x = rng.integers(0, 256, size=(12, 32, 32, 3), dtype=np.uint8)
    t = np.arange(12, dtype=np.int64) % 10
    got = list(cifar.device_batches(x, t, 5, torch.device("cpu")))
    assert [b[0].shape[0] for b in got] == [5, 5, 2] == [b[1].shape[0] for b in got]
    assert all(b[0].dtype == torch.uint8 and b[1].dtype == torch.int64 and b[0].is_contiguous() for b in got)
    assert np.array_equal(torch.cat([b[0] for b in got]).numpy(), x)
    assert np.array_equal(torch.cat([b[1] for b in got]).numpy(), t)
    assert [b[0].shape[0] for b in cifar.device_batches(x, t, 12, "cpu")] == [12]
    assert [b[0].shape[0] for b in cifar.device_batches(x, t, 64, "cpu")] == [12]
    with pytest.raises(ValueError):
        list(cifar.device_batches(x.transpose(0, 3, 1, 2), t, 5, "cpu"))
    with pytest.raises(ValueError):
        list(cifar.device_batches(x, t[:11], 5, "cpu"))
    with pytest.raises(ValueError):
        list(cifar.device_batches(x, t, 0, "cpu"))
    assert cifar.CIFAR_MEAN == (0.4914, 0.4822, 0.4465) and cifar.CIFAR_STD == (0.2023, 0.1994, 0.2010)
