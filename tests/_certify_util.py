"""Shared by tests/test_certify_cpu.py and tests/test_gpu_certify.py: the float64 stem of vAlexnet on real-valued inputs
(test infrastructure; imports oracle/)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ttnet_float as OF
from scale_imagenet_amd import certify as CF
from scale_imagenet_amd import cifar


def oracle_pre(st, x_norm: np.ndarray) -> np.ndarray:
    """float64 pooled pre-activation [n, 64, 10, 10] of normalised real-valued images [n, 3, 32, 32]: the first lines of
    ``OF.forward_valexnet`` on double tensors."""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in OF.to_torch_state(st).items()}
    h = F.relu(F.conv2d(torch.from_numpy(x_norm), sd["features.0.weight"], sd["features.0.bias"], 1, 1))
    return F.max_pool2d(OF._bn(h, sd, "features.2"), 3).numpy()


def normalise(v: np.ndarray, mean=cifar.CIFAR_MEAN, std=cifar.CIFAR_STD) -> np.ndarray:
    """Real byte levels HWC [n, 32, 32, 3] -> normalised CHW float64, with the float32 constants the plan holds."""
    a, off = CF._norm(mean, std)
    return np.ascontiguousarray(((v - off) * a).transpose(0, 3, 1, 2))
