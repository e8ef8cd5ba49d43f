"""Pure-NumPy restatement of the Spotify negative sampler (esr_philox.h, esr_spotify_sample_negatives): Philox4x32-10 as
in Random123 plus the multiply-high map to [0, T - 1).  Shared by the CPU and GPU tests; nothing here touches the library."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (any ints < 2^32; broadcast against each other) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2          # < 2^64: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def negative_indices(seed, step, num_negatives, T):
    """int64 [num_negatives]: negative i = (word (i & 3) of philox((i >> 2, step, 0, 0), (seed lo, seed hi)) * (T - 1)) >> 32."""
    seed = int(seed) & (2 ** 64 - 1)
    i = np.arange(num_negatives, dtype=np.uint64)
    counter = np.zeros((num_negatives, 4), dtype=np.uint64)
    counter[:, 0] = i >> np.uint64(2)
    counter[:, 1] = np.uint64(int(step) & 0xFFFFFFFF)
    words = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    w = words[np.arange(num_negatives), (i & np.uint64(3)).astype(np.int64)].astype(np.uint64)
    return ((w * np.uint64(T - 1)) >> S32).astype(np.int64)


def list_starts(n, next_offsets, o):
    """int offsets of every step's [album ids][artist ids] block in esr_spotify_train_steps' workspace
    (include/esr_hip.h): roundup(2 (j (n + o) + next_offsets[j]), 64) + 64 j."""
    off = np.asarray(next_offsets, dtype=np.int64)
    j = np.arange(off.size - 1, dtype=np.int64)
    return (2 * (j * (n + o) + off[:-1]) + 63) // 64 * 64 + 64 * j
