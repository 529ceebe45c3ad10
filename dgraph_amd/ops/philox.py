"""Philox4x32-10, the attention-dropout keep mask and the DropEdge keep decision
(:func:`edge_keep_mask`) in torch integer ops.

The same generator as ``csrc/kernels/philox.h`` (Salmon et al., SC'11; the Random123 /
cuRAND / torch generator), bit for bit: the fused dropout kernels
(``csrc/kernels/dot_attn_drop_f32.hip``) never store their mask, they regenerate it from
``(seed, CSR slot, head)``, and this module regenerates it once more for the CPU path of
``dot_attention(..., dropout_p=)`` and for every oracle::

    words = philox4x32_10(counter = (s & 0xffffffff, s >> 32, h >> 2, 0),
                          key     = (seed & 0xffffffff, seed >> 32))
    keep(s, h) = words[h & 3] >= thr          thr = floor(p * 2^32),  0 <= p < 1

32-bit words are held in int64 tensors masked to 32 bits (torch has no uint32 arithmetic), the
32 x 32 -> 64 products are formed from 16-bit halves so nothing overflows int64. Works on CPU
and GPU tensors alike; it is not a hot path.
"""
from __future__ import annotations

import math
from typing import Union

import torch

M32 = 0xFFFFFFFF
_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85


def _mulhilo(m: int, x: torch.Tensor):
    """``(hi, lo)`` 32-bit words of ``m * x`` for a 32-bit constant ``m`` and 32-bit ``x``."""
    t0 = m * (x & 0xFFFF)          # < 2^48
    t1 = m * (x >> 16)             # < 2^48
    low = ((t1 & 0xFFFF) << 16) + (t0 & M32)
    hi = (t1 >> 16) + (t0 >> 32) + (low >> 32)
    return hi & M32, low & M32


def philox4x32_10(counter: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
    """``counter [..., 4]`` and ``key [..., 2]`` (int64 holding 32-bit words, broadcastable in
    the leading dimensions) -> the four output words ``[..., 4]`` (int64, 32-bit values)."""
    counter, key = counter.long() & M32, key.long() & M32
    c0, c1, c2, c3 = counter.unbind(-1)
    k0, k1 = key.unbind(-1)
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c0)
        hi1, lo1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return torch.stack(torch.broadcast_tensors(c0, c1, c2, c3), -1)


def keep_threshold(p: float) -> int:
    """``floor(p * 2^32)`` for ``0 <= p < 1``."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must lie in [0, 1), got {p}")
    return int(math.floor(p * 4294967296.0))


def attn_keep_mask(seed: Union[int, torch.Tensor], num_slots: int, heads: int, p: float,
                   first_slot: int = 0, device=None) -> torch.Tensor:
    """``keep [num_slots, heads]`` (bool) of the CSR slots ``first_slot .. first_slot +
    num_slots``: the mask the kernels regenerate. ``seed``: a Python int or a 1-element int64
    tensor (the mask is then built on its device with no host sync)."""
    thr = keep_threshold(p)
    if isinstance(seed, torch.Tensor):
        device = seed.device if device is None else device
        sd = seed.reshape(()).long().to(device)
    else:
        sd = torch.tensor(int(seed), dtype=torch.int64, device=device)  # (an int64 value)
    key = torch.stack([sd & M32, (sd >> 32) & M32])
    slots = torch.arange(first_slot, first_slot + num_slots, dtype=torch.int64, device=device)
    groups = (heads + 3) // 4
    grp = torch.arange(groups, dtype=torch.int64, device=device)
    counter = torch.stack(torch.broadcast_tensors(
        (slots & M32)[:, None], (slots >> 32)[:, None], grp[None, :],
        torch.zeros((), dtype=torch.int64, device=device)), -1)      # [S, groups, 4]
    words = philox4x32_10(counter, key)                               # [S, groups, 4]
    return (words.reshape(num_slots, 4 * groups)[:, :heads] >= thr)


def edge_keep_mask(seed: Union[int, torch.Tensor], dst_ids: torch.Tensor, src_ids: torch.Tensor,
                   p: float, undirected: bool = False) -> torch.Tensor:
    """The DropEdge keep decision of the edges ``dst_ids[i] <- src_ids[i]`` (bool, their
    broadcast shape), bit for bit ``edge_keep`` of ``csrc/kernels/philox.h``::

        (a, b) = (dst, src)                          directed
        (a, b) = (min(dst, src), max(dst, src))      undirected
        words  = philox4x32_10(counter = (a & M32, a >> 32, b & M32, b >> 32),
                               key     = (seed & M32, seed >> 32))
        keep   = words[0] >= floor(p * 2^32)         0 <= p < 1;  p = 0 keeps everything

    It depends on the seed and the two non-negative int64 vertex ids alone, not on a CSR
    slot: the transposed pass regenerates it without a slot map, global ids make it the same
    on every partition, ``undirected`` gives both directions of an edge one fate, and
    parallel entries with equal ``(dst, src)`` always share one. ``seed``: a Python int or a
    1-element int64 tensor (no host sync)."""
    thr = keep_threshold(p)
    dst, src = torch.broadcast_tensors(dst_ids.long(), src_ids.long())
    device = dst.device
    if isinstance(seed, torch.Tensor):
        sd = seed.reshape(()).long().to(device)
    else:
        sd = torch.tensor(int(seed), dtype=torch.int64, device=device)
    key = torch.stack([sd & M32, (sd >> 32) & M32])
    a, b = (torch.minimum(dst, src), torch.maximum(dst, src)) if undirected else (dst, src)
    counter = torch.stack([a & M32, (a >> 32) & M32, b & M32, (b >> 32) & M32], -1)
    return philox4x32_10(counter, key)[..., 0] >= thr
