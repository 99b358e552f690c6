"""Restatement of the per-codeword CRC-32 (gf3_crc_attach / gf3_crc_check), from zlib.crc32 and
np.packbits alone.

A codeword's message of k bits is a payload of k' = k - 32 bits followed by a CRC field of 32 bits.  Payload byte b is
payload bits 8b .. 8b+7, most significant first (np.packbits: the bytes the outer code works on);
c = zlib.crc32(payload bytes) (CRC-32/IEEE: reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF);
message bit k - 32 + i is bit 31 - i of c.  k is a multiple of 8 in [40, 7936].  The arithmetic is exact: the GPU is
compared with this file byte for byte."""
import zlib

import numpy as np

CRC_BITS = 32
MIN_K, MAX_K = 40, 7936


def check_k(k):
    if k % 8 or not MIN_K <= k <= MAX_K:
        raise ValueError(f"k must be a multiple of 8 in [{MIN_K}, {MAX_K}]")


def fields(payload):
    """0/1 payload bits [n_cw, k - 32] -> the 32 bits of each row's CRC field, uint8 [n_cw, 32]."""
    packed = np.packbits(np.asarray(payload, dtype=np.uint8) & 1, axis=1)
    c = np.array([zlib.crc32(row.tobytes()) for row in packed], dtype=np.int64).reshape(-1, 1)
    return ((c >> (31 - np.arange(CRC_BITS))) & 1).astype(np.uint8)


def attach(payload, k):
    """[n_cw, k - 32] 0/1 payload bits -> uint8 [n_cw, k]: each row followed by its CRC field."""
    check_k(k)
    payload = np.asarray(payload, dtype=np.uint8).reshape(-1, k - CRC_BITS) & 1
    return np.concatenate([payload, fields(payload)], axis=1)


def check(msg, k, iters=None):
    """[n_cw, k] 0/1 message bits -> (payload [n_cw, k - 32], bad uint8 [n_cw], iters or None): bad = the field is not the
    payload's CRC; a copy of iters with v > 0 on a bad row turned into -v, every other value as it is."""
    check_k(k)
    msg = np.asarray(msg, dtype=np.uint8).reshape(-1, k) & 1
    payload = msg[:, : k - CRC_BITS].copy()
    bad = (fields(payload) != msg[:, k - CRC_BITS:]).any(axis=1).astype(np.uint8)
    if iters is None:
        return payload, bad, None
    iters = np.array(iters, dtype=np.int32).reshape(-1)
    return payload, bad, np.where((bad != 0) & (iters > 0), -iters, iters).astype(np.int32)
