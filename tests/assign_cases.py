"""Shared by the streaming-assignment tests: the numpy restatement of the packed key of include/segger_amd.h
(segger_assign_update) and the similarity values every test of it uses."""
import numpy as np
import torch

U32 = np.uint64(0xFFFFFFFF)


def assign_keys(sim, q):
    """key = (ord(sim) << 32) | (0xFFFFFFFF - q) as uint64; sim float32 [n], q sequence numbers [n]."""
    sim = np.asarray(sim, dtype=np.float32)
    with np.errstate(invalid="ignore"):                                       # a signalling NaN among the inputs
        b = (sim + np.float32(0.0)).view(np.uint32).astype(np.uint64)         # -0.0 -> +0.0
    b = np.where(np.isnan(sim), np.uint64(0x7FC00000), b)                     # one canonical NaN
    ordv = b ^ np.where((b >> np.uint64(31)) != 0, U32, np.uint64(0x80000000))
    return (ordv << np.uint64(32)) | (U32 - np.asarray(q).astype(np.uint64))


def bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def special_similarities():
    """+-0, +-1, +-inf, NaN, -NaN, a NaN with a payload, the smallest and a mid-range denormal of both signs."""
    return np.concatenate([
        np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf], dtype=np.float32),
        bits(0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000001, 0x80000001, 0x00012345, 0x80012345)])


def key_test_similarities(seed=0, n_random=2000):
    """~2000 random similarities in [-1, 1] (a quarter rounded to 1/64: exact duplicates) plus every special twice,
    shuffled."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(-1.0, 1.0, n_random).astype(np.float32)
    r[::4] = np.round(r[::4] * 64) / 64
    s = np.concatenate([r, special_similarities(), special_similarities()])
    return s[rng.permutation(s.size)]


def same(a, b):
    """torch.equal, with NaN == NaN for floating tensors (and -0.0 == +0.0, as torch.equal has it)."""
    a, b = a.cpu(), b.cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    return torch.equal(a, b)
