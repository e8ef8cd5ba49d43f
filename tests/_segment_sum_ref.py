"""The row-sparse update engine's geometry and summation order, restated in plain Python / numpy float32.

esr_optim.hip's segment_update_kernel / segment_long_kernel sum the gradient rows of every run of equal sorted ids in a
FIXED order.  Tests compare the kernels bit for bit with expected_run_sums; geom() restates row_geom + ESR_DISPATCH_ROW
(esr_common.h) so that the tests can name the instantiation a width runs in; run_pattern() builds sorted id lists whose
runs start at chosen positions modulo the chunk length.  No GPU and no torch in here.
"""
from collections import namedtuple

import numpy as np

CHUNK = 32          # kSegChunk
BLOCK = 256         # kBlock: threads per workgroup
WAVE = 64           # kWave
MAX_NCH = 4         # kMaxChunksPerLane
MAX_GRID = 2048     # kMaxGrid

Geom = namedtuple("Geom", "vec nvec G nch NCH NG")


def geom(D):
    """row_geom(D) + the template NCH ESR_DISPATCH_ROW picks (nch 3 runs as 4) + NG = row groups per workgroup.
    NCH is None for a width the engine refuses (more than MAX_NCH chunks per lane)."""
    vec = 4 if D % 4 == 0 else 1
    nvec = D // vec
    G = 1
    while G < nvec and G < WAVE:
        G <<= 1
    nch = (nvec + G - 1) // G
    NCH = None if nch > MAX_NCH else (1 if nch <= 1 else 2 if nch <= 2 else 4)
    return Geom(vec, nvec, G, nch, NCH, BLOCK // G)


def runs_of(sorted_ids):
    """[(start, length)] of the runs of equal values of a sorted list."""
    s = np.asarray(sorted_ids)
    if s.size == 0:
        return []
    starts = np.concatenate([[0], np.flatnonzero(s[1:] != s[:-1]) + 1])
    return list(zip(starts.tolist(), np.diff(np.concatenate([starts, [s.size]])).tolist()))


def chunk_bounds(p, q):
    """The chunks of the run [p, q): the head chunk ends at the first multiple of CHUNK that is at least CHUNK positions
    after p (so it holds 32 .. 63 positions), the others are aligned blocks of CHUNK; the last one ends with the run."""
    out, c = [], p
    while c < q:
        e = min(((c + 2 * CHUNK - 1) // CHUNK) * CHUNK if c == p else c + CHUNK, q)
        out.append((c, e))
        c = e
    return out


def nparts(start, length):
    return len(chunk_bounds(start, start + length))


def length_for_parts(align, parts, last=1):
    """Length of a run that starts at a position = align (mod CHUNK) and is cut into `parts` chunks, the last of which
    holds `last` positions (1 .. CHUNK); parts >= 2."""
    assert parts >= 2 and 1 <= last <= CHUNK
    head = ((align + 2 * CHUNK - 1) // CHUNK) * CHUNK - align
    return head + CHUNK * (parts - 2) + last


def _seq_sum(x):
    """left-to-right float32 sum of the rows of x (np.add.accumulate is sequential; np.sum is pairwise)"""
    return x[0].copy() if x.shape[0] == 1 else np.add.accumulate(x, axis=0, dtype=np.float32)[-1]


def expected_run_sums(ids, rows, D, scratch=False):
    """(distinct ids ascending, float32 [U, D] run sums) in the order the kernels add: a run with one chunk is its
    left-to-right sum; otherwise partial i is the left-to-right sum of chunk i, row group g in range(min(NG, nparts)) adds
    partials g, g + NG, ... in order onto zero, and the group sums are added in group order.  NG = geom(D).NG.
    scratch=True: also the gradient-row buffer as the call leaves it (the first position of every chunk of a run with
    several chunks holds that chunk's partial; every other row is untouched)."""
    ids = np.asarray(ids)
    rows = np.asarray(rows, np.float32).reshape(ids.size, D)
    NG = geom(D).NG
    order = np.argsort(ids, kind="stable")
    sids = ids[order]
    runs = runs_of(sids)
    out = np.empty((len(runs), D), np.float32)
    left = rows.copy() if scratch else None
    srows = rows[order]
    for u, (p, n) in enumerate(runs):
        if n == 1:
            out[u] = srows[p]
            continue
        bounds = chunk_bounds(p, p + n)
        if len(bounds) == 1:
            out[u] = _seq_sum(srows[p:p + n])
            continue
        parts = np.stack([_seq_sum(srows[c:e]) for c, e in bounds])
        if scratch:
            left[order[[c for c, _ in bounds]]] = parts
        used = min(NG, len(bounds))
        sums = np.zeros((used, D), np.float32)
        for j in range(0, len(bounds), NG):
            blk = parts[j:j + NG]
            sums[:blk.shape[0]] = sums[:blk.shape[0]] + blk
        out[u] = _seq_sum(sums)
    uniq = sids[[p for p, _ in runs]] if runs else sids[:0]
    return (uniq, out, left) if scratch else (uniq, out)


def run_pattern(spec, tail=0):
    """Sorted run indices (0, 0, 1, 2, 2, 2, ...) for spec = [(start position mod CHUNK, run length)]: every named run is
    preceded by as many filler runs of length 1 as it takes to start at the asked alignment; `tail` fillers follow the
    last run.  Returns (list, indices of the named runs)."""
    out, named, pos, nxt = [], [], 0, 0
    for align, length in spec:
        while pos % CHUNK != align % CHUNK:
            out.append(nxt)
            nxt += 1
            pos += 1
        out.extend([nxt] * length)
        named.append(nxt)
        nxt += 1
        pos += length
    for _ in range(tail):
        out.append(nxt)
        nxt += 1
    return np.asarray(out, np.int32), named


def assert_pattern(sorted_ids, spec):
    """every (alignment, length) of spec occurs among the runs of the SORTED list the kernel is given"""
    have = {(p % CHUNK, n) for p, n in runs_of(sorted_ids)}
    missing = [s for s in spec if (s[0] % CHUNK, s[1]) not in have]
    assert not missing, "run pattern drifted: %r missing" % (missing,)
