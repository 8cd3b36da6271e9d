"""GPU: bench.py's own contract.  A plain run times exactly --steps steps and prints only the headline;
--dump-outputs writes the logits the timed path computed in its last step; --full adds the other legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _util import ROOT, args_for, spec_and_state
from scale_imagenet_amd import synth, ttnet

pytestmark = pytest.mark.gpu

FULL_ONLY = {"serial", "roofline", "roofline_kernels", "kernel_ms_sum", "gate_path", "parity", "cpu_baseline"}


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    out = tmp_path / "dump"
    d = _bench("--gpus", "1", "--steps", "5", "--warmup", "2", "--batch", "8", "--dump-outputs", str(out))
    assert d["steps"] == 5 and d["windows"]["n"] == 1 and d["inflight"] == 2
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert not FULL_ONLY & set(d)
    y = np.load(out / "logits.npy")
    assert y.dtype == np.float32 and y.shape == (8, 1000)
    # step 4 of 5 reads input buffer 4 % 4 = 0, the images in their own order: one plain forward of them
    _, st = spec_and_state("small")
    m = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    dev = torch.device("cuda", 0)
    m = m.to(dev).eval()
    with torch.no_grad():
        want = m(torch.from_numpy(synth.synth_images(8)).to(dev)).cpu().numpy()
    assert np.abs(y - want).max() <= 1e-6


def test_full_run_keeps_the_other_legs():
    d = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8", "--full", "--no-cpu-baseline")
    assert d["steps"] == 3 and d["windows"]["n"] == 9 and d["ms_per_step"] > 0
    assert "extras_error" not in d
    assert {"serial", "roofline", "roofline_kernels", "kernel_ms_sum", "gate_path", "uint8_input", "parity"} <= set(d)
    assert d["parity"]["images"] > 0 and len(d["gate_path"]["b2048"]) > 0
