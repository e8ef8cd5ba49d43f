"""Tensor-level wrappers over the C ABI (include/esr_hip.h).

PyTorch is used for device memory and the current HIP stream only; every computation is a
libesr_hip.so call.  All functions require CUDA(ROCm) tensors and raise if the library is missing.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import ESR_BF16, ESR_F32, GLOVE_DIAGONAL, GLOVE_REFERENCE, check  # noqa: F401


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream on the current device.  torch.cuda.current_stream() builds a Stream
    object through several Python layers (~2 us, four or more times per step on launch-bound steps); the raw getter
    is one C call."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _req(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA/ROCm tensor (no CPU fallback exists)" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _table_dtype(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA/ROCm tensor (no CPU fallback exists)" % name)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if t.dtype == torch.float32:
        return ESR_F32
    if t.dtype == torch.bfloat16:
        return ESR_BF16
    raise TypeError("%s must be float32 or bfloat16, got %s" % (name, t.dtype))


def check_device_ids(ids, V):
    """Debug screen (ESR_CHECK_IDS=1): raise IndexError if any id of the device tensor is outside [0, V).
    One small launch + a host read-back, i.e. a sync -- which is why it is not on by default."""
    lib = _lib.load()
    report = torch.tensor([0, 2 ** 63 - 1], dtype=torch.int64, device=ids.device)
    check(lib.esr_check_ids(_p(ids), ids.numel(), int(V), _p(report), _stream()), "esr_check_ids")
    bad, first = (int(v) for v in report.cpu())
    if bad:
        raise IndexError("%d device-resident id(s) out of range [0, %d); first at flat position %d (value %d)"
                         % (bad, V, first, int(ids.reshape(-1)[first])))


def as_ids(x, device, check_range=None):
    """int ids (numpy / list / torch, any int dtype) -> contiguous int32 tensor on `device`.

    Host inputs are range-checked against `check_range` = V.  Device inputs are trusted (checking them forces a
    sync on the hot path) unless ESR_CHECK_IDS=1 is set in the environment: then every device id tensor is screened
    by esr_check_ids and an out-of-range id raises IndexError instead of becoming a wild read / RMW."""
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            # (an int32 contiguous device tensor -- what a training loop hands over -- passes through untouched: the two
            # no-op torch calls were ~3 us per tensor, a quarter of the host's time per step in the triplet loop at B = 8192)
            if x.dtype is not torch.int32 or not x.is_contiguous():
                x = x.to(torch.int32).contiguous()
            if check_range is not None and os.environ.get("ESR_CHECK_IDS") == "1":
                check_device_ids(x, check_range)
            return x
        x = x.numpy()
    a = np.ascontiguousarray(np.asarray(x), dtype=np.int32)
    if check_range is not None and a.size and (a.min() < 0 or a.max() >= check_range):
        raise IndexError("id out of range [0, %d): min %d max %d" % (check_range, a.min(), a.max()))
    return torch.from_numpy(a).to(device, non_blocking=True)


def as_f32(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).to(device, non_blocking=True)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


_ws_size_cache = {}


def _ws_bytes(fn_name, *args):
    key = (fn_name,) + args
    v = _ws_size_cache.get(key)
    if v is None:
        v = int(getattr(_lib.load(), fn_name)(*args))
        _ws_size_cache[key] = v
    return v


# ---------------------------------------------------------------------------------------------
def gather_rows(table, ids, out=None):
    """out[i] = table[ids[i]]  (bit-exact).  table [V, D] f32/bf16; ids int32 [n]."""
    lib = _lib.load()
    dt = _table_dtype(table, "table")
    ids = _req(ids, torch.int32, "ids")
    V, D = table.shape
    n = ids.numel()
    if out is None:
        out = torch.empty((n, D), dtype=table.dtype, device=table.device)
    check(lib.esr_gather_rows(_p(table), dt, V, D, _p(ids), n, _p(out), _stream()), "esr_gather_rows")
    return out


def unpermute_rows(rows, perm, out=None):
    """out[perm[k]] = rows[k]."""
    lib = _lib.load()
    dt = _table_dtype(rows, "rows")
    perm = _req(perm, torch.int32, "perm")
    n, D = rows.shape
    if out is None:
        out = torch.empty_like(rows)
    check(lib.esr_unpermute_rows(_p(rows), dt, D, _p(perm), n, _p(out), _stream()), "esr_unpermute_rows")
    return out


def unpermute_rows_to_f32(rows, perm, out=None):
    """out[perm[k]] = float32(rows[k]); rows may be bf16 (converted on the fly) or f32."""
    if rows.dtype == torch.float32:
        return rows if perm is None else unpermute_rows(rows, perm, out)
    lib = _lib.load()
    _req(rows, torch.bfloat16, "rows")
    n, D = rows.shape
    if out is None:
        out = torch.empty((n, D), dtype=torch.float32, device=rows.device)
    check(lib.esr_unpermute_rows_bf16_to_f32(_p(rows), D, _p(perm), n, _p(out), _stream()),
          "esr_unpermute_rows_bf16_to_f32")
    return out


def glove_forward(emb, bias, inputs):
    """(dot[B], s[B]) of Glove.__call__; the reference output is dot[None, :] + s[:, None]."""
    lib = _lib.load()
    _req(emb, torch.float32, "emb"), _req(bias, torch.float32, "bias"), _req(inputs, torch.int32, "inputs")
    V, D = emb.shape
    B = inputs.shape[1]
    dot = torch.empty(B, dtype=torch.float32, device=emb.device)
    s = torch.empty(B, dtype=torch.float32, device=emb.device)
    check(lib.esr_glove_forward(_p(emb), _p(bias), V, D, _p(inputs), B, _p(dot), _p(s), _stream()),
          "esr_glove_forward")
    return dot, s


def glove_fwd_bwd(emb, bias, inputs, target, mode=GLOVE_REFERENCE, want_grads=True, grads_at_ids=False):
    """Fused GloVe loss + per-occurrence gradients.  Returns (loss[1], grad_rows[2B, D], grad_bias[2B]).
    grads_at_ids: emb / bias are a [2B, .] copy of the looked-up rows (one row per occurrence, any order) and the
    gradient of the occurrence that read row r is written at row r."""
    lib = _lib.load()
    _req(emb, torch.float32, "emb"), _req(bias, torch.float32, "bias")
    _req(inputs, torch.int32, "inputs"), _req(target, torch.float32, "target")
    V, D = emb.shape
    B = inputs.shape[1]
    if inputs.shape[0] != 2 or target.numel() != B:
        raise ValueError("inputs must be [2, B] and target [B]")
    dev = emb.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    grad_rows = torch.empty((2 * B, D), dtype=torch.float32, device=dev) if want_grads else None
    grad_bias = torch.empty(2 * B, dtype=torch.float32, device=dev) if want_grads else None
    nb = _ws_bytes("esr_glove_workspace_bytes", B)
    ws = _ws(nb, dev)
    if grads_at_ids and want_grads:
        mode = mode | GRADS_AT_IDS
    check(lib.esr_glove_fwd_bwd(_p(emb), _p(bias), V, D, _p(inputs), _p(target), B, mode, _p(loss), _p(grad_rows),
                                _p(grad_bias), _p(ws), ws.numel(), _stream()), "esr_glove_fwd_bwd")
    return loss, grad_rows, grad_bias


GRADS_AT_IDS = 0x100  # include/esr_hip.h ESR_GRADS_AT_IDS


def glove_train_step(emb, shadow, loc, accum, bias, bias_accum, inputs, target, mode, lr, eps=1e-7, presorted=None,
                     blocks_per_cu=0, stamp=None, plan=None, long_runs=-1, start_flag=None, start_value=0):
    """One whole GloVe training step (loss + gradients + sparse Adagrad on both tables) without materialised
    gradients: esr_glove_train_step.  `emb` / `shadow` are the two buffers of the double-buffered embedding table and
    `loc` (uint8 [V]) holds each row's stamped location byte; all three are updated.  `stamp` (1 .. 127): this step's
    stamp on that table (train_state.next_stamp hands them out and clears the bytes' stamps when the counter wraps).
    presorted = (sorted_ids, perm) of inputs.reshape(-1) from segment_sort (computed ahead), else the sort runs here;
    plan = this batch's glove_plan record (needs presorted), long_runs = 0 when its hint said no run is long.
    start_flag (int32 [1] device tensor) / start_value: the update kernel announces its start there (stream_gate).
    Returns loss[1]."""
    lib = _lib.load()
    dt = _table_dtype(emb, "emb")  # f32, or bf16 rows (both buffers) with fp32 accumulator and bias tables
    if _table_dtype(shadow, "shadow") != dt:
        raise TypeError("emb and shadow must have the same dtype")
    for name, t in (("accum", accum), ("bias", bias), ("bias_accum", bias_accum), ("target", target)):
        _req(t, torch.float32, name)
    _req(loc, torch.uint8, "loc"), _req(inputs, torch.int32, "inputs")
    if stamp is None:
        raise ValueError("glove_train_step needs the step's stamp (train_state.next_stamp(row_versions))")
    V, D = emb.shape
    B = inputs.shape[1]
    if inputs.shape[0] != 2 or target.numel() != B:
        raise ValueError("inputs must be [2, B] and target [B]")
    if shadow.shape != emb.shape or accum.shape != emb.shape or loc.numel() != V or bias.numel() != V or \
            bias_accum.numel() != V:
        raise ValueError("shadow / accum / loc / bias shapes do not match the embedding table")
    loss = torch.empty(1, dtype=torch.float32, device=emb.device)
    ws = _ws(_ws_bytes("esr_glove_step_workspace_bytes", B, D), emb.device)
    sid = perm = None
    if presorted is not None:
        sid, perm = _req(presorted[0], torch.int32, "sorted_ids"), _req(presorted[1], torch.int32, "perm")
        if sid.numel() != 2 * B or perm.numel() != 2 * B:
            raise ValueError("presorted ids / perm must have 2 B entries")
    if plan is not None and (plan.dtype != torch.uint8 or plan.numel() < _ws_bytes("esr_glove_plan_bytes", B)):
        raise ValueError("plan must be the uint8 record glove_plan made for a batch of this size")
    check(lib.esr_glove_train_step(_p(emb), _p(shadow), _p(loc), _p(accum), _p(bias), _p(bias_accum), V, dt, D, _p(inputs),
                                   _p(target), B, mode, float(lr), float(eps), int(stamp), _p(sid), _p(perm), _p(plan),
                                   int(long_runs), int(blocks_per_cu), _p(start_flag), int(start_value) & 0xFFFFFFFF,
                                   _p(loss), _p(ws), ws.numel(), _stream()),
          "esr_glove_train_step")
    return loss


def stream_gate(flag, value, timeout_us=1_000_000):
    """Hold the CURRENT stream (one sleeping wave) until the device word flag[0] has reached `value` (sequence numbers,
    wrap-safe) or timeout_us have passed: esr_stream_gate."""
    lib = _lib.load()
    if not (flag.is_cuda and flag.dtype == torch.int32 and flag.numel() >= 1):
        raise ValueError("stream_gate: flag must be an int32 device tensor")
    check(lib.esr_stream_gate(_p(flag), int(value) & 0xFFFFFFFF, int(timeout_us), _stream()), "esr_stream_gate")


def _aligned_bytes(nbytes, device, align=256):
    """ZEROED uint8 tensor of nbytes whose data pointer is `align`-aligned (torch's allocator hands out 512-byte blocks).
    Plan buffers come from here: the direct triplet plan's long-run counter is tagged with the plan call's generation
    (esr_triplet_step.hip) -- a fresh buffer must not hold a word that happens to carry a live tag."""
    t = torch.zeros(nbytes + align, dtype=torch.uint8, device=device)
    off = (-t.data_ptr()) % align
    return t[off:off + nbytes]


def glove_plan(inputs_list, targets_list, sorted_ids, perm, hints=None, gen=0):
    """Plan records of up to eight coming GloVe batches by one launch (esr_glove_plan): inputs_list[b] int32 [2, B],
    targets_list[b] f32 [B], sorted_ids / perm int32 [nb, 2B].  Returns a uint8 [nb, plan_bytes] tensor (row b feeds
    exactly one glove_train_step).  hints: optional int32 [nb] device tensor that receives `gen` where list b has a run
    longer than a chunk."""
    lib = _lib.load()
    nb = len(inputs_list)
    B = inputs_list[0].shape[1]
    for i, t in zip(inputs_list, targets_list):
        _req(i, torch.int32, "inputs"), _req(t, torch.float32, "target")
        if i.shape != (2, B) or t.numel() != B:
            raise ValueError("every batch of a plan group must be [2, B] / [B] with the same B")
    _req(sorted_ids, torch.int32, "sorted_ids"), _req(perm, torch.int32, "perm")
    if sorted_ids.numel() != nb * 2 * B or perm.numel() != nb * 2 * B:
        raise ValueError("sorted_ids / perm must be [nb, 2B]")
    pb = _ws_bytes("esr_glove_plan_bytes", B)
    plans = _aligned_bytes(nb * pb, inputs_list[0].device).view(nb, pb)
    ip = (ctypes.c_void_p * nb)(*[i.data_ptr() for i in inputs_list])
    tp = (ctypes.c_void_p * nb)(*[t.data_ptr() for t in targets_list])
    check(lib.esr_glove_plan(ip, tp, nb, B, _p(sorted_ids), _p(perm), _p(plans), _p(hints), int(gen), _stream()),
          "esr_glove_plan")
    return plans


def unique_by_owner(id_tensors, world, local_rows, offsets=None):
    """The distinct rows of an occurrence list, routed by owner (esr_unique_by_owner): id_tensors = int32 segments (or one
    tensor), offsets = their virtual-row offsets.  Returns (ulocal [n] -- first sum(ucounts) entries valid --, ucounts
    int64 [world] on the device, uidx [n], sorted_uidx [n], perm [n])."""
    lib = _lib.load()
    if isinstance(id_tensors, torch.Tensor):
        id_tensors = [id_tensors.reshape(-1)]
    offsets = list(offsets) if offsets is not None else [0] * len(id_tensors)
    for t in id_tensors:
        _req(t, torch.int32, "ids")
    dev = id_tensors[0].device
    k = len(id_tensors)
    counts = [int(t.numel()) for t in id_tensors]
    n = sum(counts)
    ulocal = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    uidx, sorted_uidx, perm = torch.empty_like(ulocal), torch.empty_like(ulocal), torch.empty_like(ulocal)
    ucounts = torch.empty(world, dtype=torch.int64, device=dev)
    ws = _ws(_ws_bytes("esr_unique_by_owner_workspace_bytes", n), dev)
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in id_tensors])
    cnt = (ctypes.c_int64 * k)(*counts)
    off = (ctypes.c_int64 * k)(*[int(x) for x in offsets])
    check(lib.esr_unique_by_owner(ptrs, cnt, off, k, int(world), int(local_rows), _p(ulocal), _p(uidx), _p(sorted_uidx),
                                  _p(perm), _p(ucounts), _p(ws), ws.numel(), _stream()), "esr_unique_by_owner")
    return ulocal[:n], ucounts, uidx[:n], sorted_uidx[:n], perm[:n]


def segment_sum_rows(rows_out, sorted_ids, perm, grad_rows):
    """[rows_out, D]: row u = the sum of grad_rows[perm[p]] over the positions p with sorted_ids[p] == u (every u in
    [0, rows_out) must occur: the distinct-row index of unique_by_owner).  Overwrites grad_rows."""
    lib = _lib.load()
    _req(sorted_ids, torch.int32, "sorted_ids"), _req(perm, torch.int32, "perm"), _req(grad_rows, torch.float32, "grad_rows")
    grad_rows = grad_rows.reshape(grad_rows.shape[0], -1)
    D = grad_rows.shape[1]
    out = torch.empty((int(rows_out), D), dtype=torch.float32, device=grad_rows.device)
    check(lib.esr_segment_sum_rows(_p(out), int(rows_out), D, _p(sorted_ids), _p(perm), sorted_ids.numel(), _p(grad_rows),
                                   _stream()), "esr_segment_sum_rows")
    return out


def topk_columns(scores, k):
    """(values [T, k], rows [T, k]) of the k largest entries of every column of scores [V, T], best first, ties as the
    stable ascending argsort orders them (the higher row counts as larger): esr_topk_columns, k <= 1024."""
    lib = _lib.load()
    _req(scores, torch.float32, "scores")
    V, T_ = scores.shape
    out_s = torch.empty((T_, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((T_, k), dtype=torch.int32, device=scores.device)
    check(lib.esr_topk_columns(_p(scores), V, T_, int(k), _p(out_s), _p(out_i), _stream()), "esr_topk_columns")
    return out_s, out_i


def long_run_hint(sorted_ids, chunk, hint, gen):
    """hint[0] = gen when sorted_ids has a run of equal ids longer than `chunk` positions (esr_long_run_hint); `hint` is
    an int32 tensor on the device or in pinned host memory."""
    lib = _lib.load()
    _req(sorted_ids, torch.int32, "sorted_ids")
    if hint.dtype != torch.int32 or not (hint.is_cuda or hint.is_pinned()):
        raise TypeError("hint must be an int32 tensor on the device or in pinned host memory")
    check(lib.esr_long_run_hint(_p(sorted_ids), sorted_ids.numel(), int(chunk), hint.data_ptr(), int(gen), _stream()),
          "esr_long_run_hint")


def triplet_plan(id_lists, Vs, sorted_ids, perm, hints=None, gen=0):
    """Plan records of up to eight coming triplet batches by one launch (esr_triplet_plan): id_lists[b] = (scene, pos,
    neg) int32 [B] each, sorted_ids / perm int32 [nb, 3B].  Returns a uint8 [nb, plan_bytes] tensor."""
    lib = _lib.load()
    nb = len(id_lists)
    B = id_lists[0][0].numel()
    flat = []
    for trip in id_lists:
        for t in trip:
            _req(t, torch.int32, "ids")
            if t.numel() != B:
                raise ValueError("every id list of a plan group must have B entries")
            flat.append(t.data_ptr())
    _req(sorted_ids, torch.int32, "sorted_ids"), _req(perm, torch.int32, "perm")
    if sorted_ids.numel() != nb * 3 * B or perm.numel() != nb * 3 * B:
        raise ValueError("sorted_ids / perm must be [nb, 3B]")
    pb = _ws_bytes("esr_triplet_plan_bytes", B)
    plans = _aligned_bytes(nb * pb, id_lists[0][0].device).view(nb, pb)
    ptrs = (ctypes.c_void_p * (3 * nb))(*flat)
    check(lib.esr_triplet_plan(ptrs, nb, B, int(Vs), _p(sorted_ids), _p(perm), _p(plans), _p(hints), int(gen),
                               _stream()), "esr_triplet_plan")
    return plans


def triplet_direct_mode():
    """True (default) when the one-pass triplet step walks the TRIPLETS and steps rows in place (esr_triplet_step.hip,
    "DIRECT mode"); ESR_TRIPLET_STEP=stamped: the double-buffered walk over the sorted occurrences of rounds 2-3."""
    return not os.environ.get("ESR_TRIPLET_STEP", "direct").startswith("s")


def triplet_train_step(scene, scene_shadow, scene_loc, scene_accum, product, product_shadow, product_loc,
                       product_accum, scene_ids, pos_ids, neg_ids, regularization, batch_size, lr, eps=1e-7,
                       presorted=None, stamp=None, plan=None, long_runs=-1):
    """One whole Shop-The-Look training step (triplet loss + on-chip gradients + sparse Adagrad on both double-buffered
    towers): esr_triplet_train_step.  `stamp`: this step's stamp on both towers (train_state.next_stamp).  presorted =
    (sorted virtual ids, perm) of [scene ; Vs + pos ; Vs + neg] from segment_sort_multi, else the sort runs here; plan /
    long_runs as for glove_train_step (triplet_plan).  Returns loss[1]."""
    lib = _lib.load()
    direct = triplet_direct_mode()  # rows stepped in place: no second buffers, location bytes or stamp
    dt = _table_dtype(scene, "scene")   # f32, or bf16 rows with fp32 accumulators (direct mode only)
    if _table_dtype(product, "product") != dt:
        raise TypeError("scene and product towers must have the same dtype")
    if dt != ESR_F32 and not direct:
        raise TypeError("bf16 towers need the direct step (ESR_TRIPLET_STEP=stamped is set)")
    for name, t in (("scene_accum", scene_accum), ("product_accum", product_accum)):
        _req(t, torch.float32, name)
    if not direct or scene_shadow is not None:
        _req(scene_shadow, torch.float32, "scene_shadow"), _req(product_shadow, torch.float32, "product_shadow")
        _req(scene_loc, torch.uint8, "scene_loc"), _req(product_loc, torch.uint8, "product_loc")
    for name, t in (("scene_ids", scene_ids), ("pos_ids", pos_ids), ("neg_ids", neg_ids)):
        _req(t, torch.int32, name)
    if stamp is None:
        if not direct:
            raise ValueError("triplet_train_step needs the step's stamp (train_state.next_stamp(row_versions...))")
        stamp = 1
    Vs, D = scene.shape
    Vp = product.shape[0]
    B = scene_ids.numel()
    if product.shape[1] != D or pos_ids.numel() != B or neg_ids.numel() != B:
        raise ValueError("tower dims / id counts differ")
    if scene_accum.shape != scene.shape or product_accum.shape != product.shape:
        raise ValueError("accumulator shapes do not match their towers")
    if scene_shadow is not None and (scene_shadow.shape != scene.shape or scene_loc.numel() != Vs or
                                     product_shadow.shape != product.shape or product_loc.numel() != Vp):
        raise ValueError("shadow / loc shapes do not match their towers")
    sid = perm = None
    if presorted is not None:
        sid, perm = _req(presorted[0], torch.int32, "sorted_ids"), _req(presorted[1], torch.int32, "perm")
        if sid.numel() != 3 * B or perm.numel() != 3 * B:
            raise ValueError("presorted ids / perm must have 3 B entries")
    if plan is not None and (plan.dtype != torch.uint8 or plan.numel() < _ws_bytes("esr_triplet_plan_bytes", B)):
        raise ValueError("plan must be the uint8 record triplet_plan made for a batch of this size")
    loss = torch.empty(1, dtype=torch.float32, device=scene.device)
    ws = _ws(_ws_bytes("esr_triplet_step_workspace_bytes", B, D), scene.device)
    check(lib.esr_triplet_train_step(_p(scene), _p(scene_shadow), _p(scene_loc), _p(scene_accum), Vs, _p(product),
                                     _p(product_shadow), _p(product_loc), _p(product_accum), Vp, dt, D, _p(scene_ids),
                                     _p(pos_ids), _p(neg_ids), B, float(regularization), float(batch_size), float(lr),
                                     float(eps), int(stamp), _p(sid), _p(perm), _p(plan), int(long_runs), _p(loss),
                                     _p(ws), ws.numel(), _stream()),
          "esr_triplet_train_step")
    return loss


def rows_consolidate(primary, shadow, loc):
    """Copy the rows of a double-buffered table whose current value lives in `shadow` (loc[row] == 1) back into
    `primary` and clear their bytes: afterwards `primary` is the plain [V, D] table."""
    lib = _lib.load()
    dt = _table_dtype(primary, "primary")
    if _table_dtype(shadow, "shadow") != dt:
        raise TypeError("primary and shadow must have the same dtype")
    _req(loc, torch.uint8, "loc")
    V, D = primary.shape
    check(lib.esr_rows_consolidate(_p(primary), _p(shadow), _p(loc), V, dt, D, _stream()), "esr_rows_consolidate")


def rows_restamp(loc):
    """Forget the step stamps of a double-buffered table's location bytes (bit 0, the location, stays): run when the
    caller's stamp counter wraps (esr_rows_restamp; train_state.next_stamp does)."""
    lib = _lib.load()
    _req(loc, torch.uint8, "loc")
    check(lib.esr_rows_restamp(_p(loc), loc.numel(), _stream()), "esr_rows_restamp")


def triplet_fwd_bwd(scene_table, pos_table, neg_table, scene_ids, pos_ids, neg_ids, B, regularization, batch_size,
                    with_reg=True, want_grads=True, want_scores=True, grads_at_ids=False):
    """Fused STL head.  ids may be None (= row b).  Returns (loss[1], pos_score, neg_score, g_s, g_p, g_n);
    the three gradients are consecutive slices of one [3B, D] buffer (``g_s._base``).
    grads_at_ids: the three "tables" are ONE [3B, D] copy of the looked-up rows (one row per occurrence, any order)
    and every gradient row is written at the row its table row came from: returns g_s = that [3B, D] buffer,
    g_p = g_n = None."""
    lib = _lib.load()
    for name, t in (("scene_table", scene_table), ("pos_table", pos_table), ("neg_table", neg_table)):
        _req(t, torch.float32, name)
    for name, t in (("scene_ids", scene_ids), ("pos_ids", pos_ids), ("neg_ids", neg_ids)):
        if t is not None:
            _req(t, torch.int32, name)
    Vs, D = scene_table.shape
    Vp, Vn = pos_table.shape[0], neg_table.shape[0]
    if pos_table.shape[1] != D or neg_table.shape[1] != D:
        raise ValueError("tower dims differ")
    dev = scene_table.device
    f32 = dict(dtype=torch.float32, device=dev)
    loss = torch.empty(1, **f32)
    ps = torch.empty(B, **f32) if want_scores else None
    ns = torch.empty(B, **f32) if want_scores else None
    # scene / pos / neg gradient rows share one [3B, D] buffer ([scene ; pos ; neg]): the optimizer consumes
    # them as a single occurrence list (``g_s._base``; ``g_s._base[B:]`` = the product rows) with no copy.
    gall = torch.empty((3 * B, D), **f32) if want_grads else None
    flags = int(bool(with_reg))
    if grads_at_ids and want_grads:
        flags |= GRADS_AT_IDS
        gs = gp = gn = gall
    else:
        gs = gall[:B] if want_grads else None
        gp = gall[B:2 * B] if want_grads else None
        gn = gall[2 * B:] if want_grads else None
    ws = _ws(_ws_bytes("esr_triplet_workspace_bytes", B), dev)
    check(lib.esr_triplet_fwd_bwd(_p(scene_table), Vs, _p(pos_table), Vp, _p(neg_table), Vn, D, _p(scene_ids),
                                  _p(pos_ids), _p(neg_ids), B, float(regularization), float(batch_size),
                                  flags, _p(loss), _p(ps), _p(ns), _p(gs), _p(gp), _p(gn), _p(ws),
                                  ws.numel(), _stream()), "esr_triplet_fwd_bwd")
    if grads_at_ids and want_grads:
        return loss, ps, ns, gall, None, None
    return loss, ps, ns, gs, gp, gn


INBATCH_PRECISIONS = ("auto", "f32", "bf16x3", "f16x2")
INBATCH_F16X2_MAX_B = 16384  # esr_inbatch2h.hip keeps the B x B probabilities between its two passes


def _inbatch_auto_split():
    """What "auto" resolves to where both split-precision paths apply (ESR_INBATCH_AUTO=bf16x3 keeps the older one)."""
    import os
    v = os.environ.get("ESR_INBATCH_AUTO", "f16x2")
    if v not in ("f16x2", "bf16x3"):
        raise ValueError("ESR_INBATCH_AUTO must be f16x2 or bf16x3")
    return v


def inbatch_split_path(precision, B, D, bf16_tables=False):
    """The split-precision MFMA path `precision` selects for a [B, D] in-batch head: "f16x2", "bf16x3" or None (exact
    f32).  f16x2: two fp16 planes per operand, three MFMAs per product (esr_inbatch2h.hip; fp32 rows, B <= 16384);
    bf16x3: three bf16 planes, six MFMAs (esr_inbatch3.hip; also bf16 tables, where only one plane is live).  Both work
    on 128-column tiles: D <= 128, a multiple of 4 (narrower rows are zero-padded); "auto" takes them from D = 64 up
    (ESR_INBATCH_SPLIT_MIN_D), the exact-f32 kernel's own 32- / 64-column tiles below."""
    if precision not in INBATCH_PRECISIONS:
        raise ValueError("precision must be one of %s" % (INBATCH_PRECISIONS,))
    shape_ok = D % 4 == 0 and 0 < D <= 128 and B % 128 == 0 and B > 0
    # bf16 tables (round 5): the fp16 entry points run their ONE-plane kernels on them (a bf16 element is exact in one
    # fp16 plane of x * 2^e): six GEMMs with S^T recomputed by pass C, against eight on the bf16 x 3 one-plane kernels.
    # ESR_INBATCH_BF16_TABLES=bf16x3 keeps the older path.
    h_ok = shape_ok and B <= INBATCH_F16X2_MAX_B and \
        (not bf16_tables or os.environ.get("ESR_INBATCH_BF16_TABLES", "f16") != "bf16x3")
    if precision == "f32":
        return None
    if precision == "bf16x3":
        if not shape_ok:
            raise ValueError("precision='bf16x3' needs D <= 128 (a multiple of 4) and B %% 128 == 0 (got B=%d, D=%d)"
                             % (B, D))
        return "bf16x3"
    if precision == "f16x2":
        if not h_ok:
            raise ValueError("precision='f16x2' needs D <= 128 (a multiple of 4), B %% 128 == 0 and B <= %d "
                             "(got B=%d, D=%d)" % (INBATCH_F16X2_MAX_B, B, D))
        return "f16x2"
    if not shape_ok or D < int(os.environ.get("ESR_INBATCH_SPLIT_MIN_D", "64")):
        return None
    return "f16x2" if h_ok and _inbatch_auto_split() == "f16x2" else "bf16x3"


def inbatch_softmax_fwd_bwd(Q, C, scale, regularization, batch_size, precision="auto", pass_c_forms=None):
    """In-batch-negative softmax on the matrix cores.  Returns (loss[1], lse[B], gQ, gC).

    precision "f32": exact-f32 MFMA (v_mfma_f32_32x32x2_f32).  "bf16x3": f32-equivalent products from three
    exact bf16 planes per operand (six v_mfma_f32_32x32x16_bf16 per block, error <= 2^-23 per product; needs
    D == 128 and B % 128 == 0).  "f16x2": two scaled fp16 planes per operand (three v_mfma_f32_32x32x16_f16 per block,
    error <= ~2^-22 per product; also B <= 16384).  "auto": f16x2 where it applies, else bf16x3, else f32.  All hold
    the 1e-5 bound."""
    lib = _lib.load()
    _req(Q, torch.float32, "Q"), _req(C, torch.float32, "C")
    B, D = Q.shape
    if C.shape != Q.shape:
        raise ValueError("Q and C must have the same shape")
    path = inbatch_split_path(precision, B, D)
    if pass_c_forms is not None:  # checked before anything is launched: the library copies 8 int32 into it
        if path != "f16x2":
            raise ValueError("pass_c_forms: only the f16x2 path has them (this call took %r)" % path)
        _req(pass_c_forms, torch.int32, "pass_c_forms")
        if pass_c_forms.numel() < 8:
            raise ValueError("pass_c_forms must hold at least 8 int32, got %d" % pass_c_forms.numel())
    dev = Q.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    lse = torch.empty(B, dtype=torch.float32, device=dev)
    gQC = torch.empty((2 * B, D), dtype=torch.float32, device=dev)  # [gQ ; gC]: one occurrence list downstream
    gQ, gC = gQC[:B], gQC[B:]
    if path == "f16x2":
        ws = _ws(_ws_bytes("esr_inbatch2h_workspace_bytes", B, D), dev)
        fn, name = lib.esr_inbatch_softmax_fwd_bwd_f16x2, "esr_inbatch_softmax_fwd_bwd_f16x2"
    elif path == "bf16x3":
        ws = _ws(_ws_bytes("esr_inbatch3_workspace_bytes", B, D), dev)
        fn, name = lib.esr_inbatch_softmax_fwd_bwd_bf16x3, "esr_inbatch_softmax_fwd_bwd_bf16x3"
    else:
        ws = _ws(_ws_bytes("esr_inbatch_workspace_bytes", B, D), dev)
        fn, name = lib.esr_inbatch_softmax_fwd_bwd, "esr_inbatch_softmax_fwd_bwd"
    check(fn(_p(Q), _p(C), B, D, float(scale), float(regularization), float(batch_size), _p(loss), _p(lse), _p(gQ),
             _p(gC), _p(ws), ws.numel(), _stream()), name)
    if pass_c_forms is not None:  # diagnostics: which form pass C took per pass-Q split (include/esr_hip.h)
        check(lib.esr_inbatch2h_pass_c_forms(_p(ws), ws.numel(), B, _p(pass_c_forms), _stream()),
              "esr_inbatch2h_pass_c_forms")
    return loss, lse, gQ, gC


# ---------------------------------------------------------------------------------------------
def segment_sort(ids, V, out=None):
    """Stable sort of occurrence ids.  Returns (sorted_ids, perm) with sorted_ids == ids[perm]; `out` = a pair of int32
    tensors of ids' size to sort into (a caller that recycles its buffers)."""
    lib = _lib.load()
    ids = _req(ids, torch.int32, "ids")
    n = ids.numel()
    if out is not None:
        sorted_ids, perm = out
        _req(sorted_ids, torch.int32, "out[0]"), _req(perm, torch.int32, "out[1]")
        if sorted_ids.numel() != n or perm.numel() != n:
            raise ValueError("segment_sort: out tensors must have ids' size")
    else:
        sorted_ids = torch.empty_like(ids)
        perm = torch.empty_like(ids)
    ws = _ws(_ws_bytes("esr_segment_sort_workspace_bytes", n), ids.device)
    check(lib.esr_segment_sort_ids(_p(ids), n, V, _p(sorted_ids), _p(perm), _p(ws), ws.numel(), _stream()),
          "esr_segment_sort_ids")
    return sorted_ids, perm


def _id_segments(id_tensors, offsets):
    """The (ptrs, counts, offsets) host arrays that the sort and bucket entry points take for the virtual list
    [ids_0 + offsets[0] ; ids_1 + offsets[1] ; ...].  Returns (ptrs, cnt, off, counts, n, device)."""
    for t in id_tensors:
        _req(t, torch.int32, "ids")
    counts = [int(t.numel()) for t in id_tensors]
    return ptr_array(id_tensors), i64_array(counts), i64_array(offsets), counts, sum(counts), id_tensors[0].device


def _id_segments_batched(id_lists, offsets):
    """_id_segments for the lists of several batches (same segment lengths in every batch): ptrs is the flattened
    [batch][segment] array, the counts are one list's.  Returns (ptrs, cnt, off, counts, n, device)."""
    counts = [int(t.numel()) for t in id_lists[0]]
    for segs in id_lists:
        if [int(t.numel()) for t in segs] != counts:
            raise ValueError("every batch must have the same segment lengths")
    ptrs, _, off, _, _, dev = _id_segments([t for segs in id_lists for t in segs], offsets)
    return ptrs, i64_array(counts), off, counts, sum(counts), dev


def segment_sort_multi(id_tensors, offsets, V):
    """Stable sort of the virtual list [ids_0 + offsets[0] ; ids_1 + offsets[1] ; ...] without materialising it.
    Returns (sorted virtual ids, perm)."""
    lib = _lib.load()
    ptrs, cnt, off, counts, n, dev = _id_segments(id_tensors, offsets)
    sorted_ids = torch.empty(n, dtype=torch.int32, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    ws = _ws(_ws_bytes("esr_segment_sort_workspace_bytes", n), dev)
    check(lib.esr_segment_sort_ids_multi(ptrs, cnt, off, len(counts), V, _p(sorted_ids), _p(perm), _p(ws), ws.numel(),
                                         _stream()), "esr_segment_sort_ids_multi")
    return sorted_ids, perm


def sparse_adagrad(table, accum, sorted_ids, perm, grad_rows, lr, eps=1e-7):
    """In-place row-sparse Adagrad on `table` / `accum` for the rows named by sorted_ids."""
    lib = _lib.load()
    dt = _table_dtype(table, "table")
    _req(accum, torch.float32, "accum"), _req(grad_rows, torch.float32, "grad_rows")
    V = table.shape[0]
    D = table.shape[1] if table.dim() > 1 else 1
    n = sorted_ids.numel()
    if grad_rows.numel() != n * D or accum.numel() != table.numel():
        raise ValueError("shape mismatch: grad_rows %s, table %s, accum %s, n %d" %
                         (tuple(grad_rows.shape), tuple(table.shape), tuple(accum.shape), n))
    check(lib.esr_sparse_adagrad_scatter(_p(table), dt, _p(accum), V, D, _p(sorted_ids), _p(perm), n, _p(grad_rows),
                                         float(lr), float(eps), _stream()), "esr_sparse_adagrad_scatter")


def concat_offset_ids(id_tensors, offsets):
    """[ids_0 + offsets[0] ; ids_1 + offsets[1] ; ...] as one int32 tensor (virtual rows of concatenated tables)."""
    lib = _lib.load()
    n = len(id_tensors)
    for t in id_tensors:
        _req(t, torch.int32, "ids")
    counts = [int(t.numel()) for t in id_tensors]
    out = torch.empty(sum(counts), dtype=torch.int32, device=id_tensors[0].device)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in id_tensors])
    cnt = (ctypes.c_int64 * n)(*counts)
    off = (ctypes.c_int64 * n)(*[int(o) for o in offsets])
    check(lib.esr_concat_offset_ids(ptrs, cnt, off, n, _p(out), _stream()), "esr_concat_offset_ids")
    return out


def i64_array(values):
    """host int64 array for the count / offset arguments of the multi-table and sharded calls"""
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _fused_tables(tables, row_offsets, table_dtype=None, **states):
    """What the calls on several same-width tables addressed by virtual rows share.  states = one list of fp32 tensors per
    state plane, by name (accumulator=[...]): one per table, of its size.  The tables must share a dtype (table_dtype, if
    given) and D.  Returns (dtype code, D, table pointers, one pointer array per state plane ..., row offsets)."""
    if table_dtype is not None:
        for t in tables:
            _req(t, table_dtype, "table")
    dts = {_table_dtype(t, "table") for t in tables}
    if len(dts) != 1:
        raise TypeError("fused tables must share a dtype")
    if len(row_offsets) != len(tables) + 1:
        raise ValueError("row_offsets must hold one entry more than there are tables")
    width = lambda t: t.shape[1] if t.dim() > 1 else 1  # noqa: E731
    D = width(tables[0])
    what = " and have matching %ss" % "s / ".join(states) if states else ""
    if any(width(t) != D for t in tables) or any(len(plane) != len(tables) for plane in states.values()):
        raise ValueError("fused tables must share D" + what)
    for name, plane in states.items():
        for t, a in zip(tables, plane):
            _req(a, torch.float32, name)
            if a.numel() != t.numel():
                raise ValueError("fused tables must share D" + what)
    return (dts.pop(), D, ptr_array(tables), *map(ptr_array, states.values()), i64_array(row_offsets))


def gather_rows_multi(tables, row_offsets, vids, out=None):
    """out[i] = tables[t][vids[i] - row_offsets[t]] for virtual rows of several same-width tables."""
    lib = _lib.load()
    dt, D, tp, ro = _fused_tables(tables, row_offsets)
    vids = _req(vids, torch.int32, "vids")
    n = vids.numel()
    if out is None:
        out = torch.empty((n, D), dtype=tables[0].dtype, device=vids.device)
    check(lib.esr_gather_rows_multi(tp, ro, len(tables), dt, D, _p(vids), n, _p(out), _stream()), "esr_gather_rows_multi")
    return out


def sparse_adagrad_multi(tables, accums, row_offsets, sorted_vids, perm, grad_rows, lr, eps=1e-7, long_runs=-1):
    """One launch of row-sparse Adagrad over several same-width tables addressed by virtual rows.  long_runs = 0: the
    caller knows (long_run_hint with chunk 32) that no id has a run the head chunk cannot hold -- the long-run launch
    is skipped."""
    lib = _lib.load()
    dt, D, tp, ap, ro = _fused_tables(tables, row_offsets, accumulator=accums)
    _req(grad_rows, torch.float32, "grad_rows")
    check(lib.esr_sparse_adagrad_scatter_multi(tp, ap, ro, len(tables), dt, D, _p(sorted_vids), _p(perm), sorted_vids.numel(),
                                               _p(grad_rows), float(lr), float(eps), int(long_runs), _stream()),
          "esr_sparse_adagrad_scatter_multi")


def sparse_sgd(table, sorted_ids, perm, grad_rows, lr):
    lib = _lib.load()
    dt = _table_dtype(table, "table")
    _req(grad_rows, torch.float32, "grad_rows")
    V = table.shape[0]
    D = table.shape[1] if table.dim() > 1 else 1
    n = sorted_ids.numel()
    check(lib.esr_sparse_sgd_scatter(_p(table), dt, V, D, _p(sorted_ids), _p(perm), n, _p(grad_rows), float(lr),
                                     _stream()), "esr_sparse_sgd_scatter")


def dense_momentum_decay(param, trace, lr, momentum):
    """In place over the whole table: trace *= momentum ; param -= lr * trace (the decay half of optax.sgd)."""
    lib = _lib.load()
    _req(param, torch.float32, "param"), _req(trace, torch.float32, "trace")
    check(lib.esr_dense_momentum_decay(_p(param), _p(trace), param.numel(), float(lr), float(momentum), _stream()),
          "esr_dense_momentum_decay")


def sparse_momentum(table, trace, sorted_ids, perm, grad_rows, lr):
    """In place on the touched rows: trace[row] += g ; table[row] -= lr * g (duplicates summed first)."""
    lib = _lib.load()
    _req(table, torch.float32, "table"), _req(trace, torch.float32, "trace"), _req(grad_rows, torch.float32, "grad_rows")
    V = table.shape[0]
    D = table.shape[1] if table.dim() > 1 else 1
    check(lib.esr_sparse_momentum_scatter(_p(table), _p(trace), V, D, _p(sorted_ids), _p(perm), sorted_ids.numel(),
                                          _p(grad_rows), float(lr), _stream()), "esr_sparse_momentum_scatter")


def momentum_catchup_rows(table, trace, last, ids, modulus, step, lr, momentum):
    """Lazy optax.sgd(lr, momentum): bring the rows ids % modulus (modulus 0: ids) up to step - 1 and mark them `step`."""
    lib = _lib.load()
    _req(table, torch.float32, "table"), _req(trace, torch.float32, "trace"), _req(last, torch.int32, "last")
    ids = _req(ids, torch.int32, "ids")
    V, D = table.shape
    check(lib.esr_momentum_catchup_rows(_p(table), _p(trace), _p(last), V, D, _p(ids), ids.numel(), int(modulus), int(step),
                                        float(lr), float(momentum), _stream()), "esr_momentum_catchup_rows")


def sparse_momentum_step(table, trace, sorted_ids, perm, grad_rows, lr, momentum):
    """In place on the touched rows: trace = g + momentum * trace ; table -= lr * trace (duplicates summed first)."""
    lib = _lib.load()
    _req(table, torch.float32, "table"), _req(trace, torch.float32, "trace"), _req(grad_rows, torch.float32, "grad_rows")
    V, D = table.shape
    check(lib.esr_sparse_momentum_step(_p(table), _p(trace), V, D, _p(sorted_ids), _p(perm), sorted_ids.numel(),
                                       _p(grad_rows), float(lr), float(momentum), _stream()), "esr_sparse_momentum_step")


def sparse_momentum_step_multi(tables, traces, row_offsets, sorted_vids, perm, grad_rows, lr, momentum):
    """sparse_momentum_step over several same-width f32 tables addressed by virtual rows (one sort, one launch pair)."""
    lib = _lib.load()
    _, D, tp, ap, ro = _fused_tables(tables, row_offsets, torch.float32, trace=traces)
    _req(grad_rows, torch.float32, "grad_rows")
    check(lib.esr_sparse_momentum_step_multi(tp, ap, ro, len(tables), D, _p(sorted_vids), _p(perm), sorted_vids.numel(),
                                             _p(grad_rows), float(lr), float(momentum), _stream()),
          "esr_sparse_momentum_step_multi")


def momentum_flush(table, trace, last, step, lr, momentum):
    """Bring every row of a lazily updated table up to `step`."""
    lib = _lib.load()
    _req(table, torch.float32, "table"), _req(trace, torch.float32, "trace"), _req(last, torch.int32, "last")
    V, D = table.shape
    check(lib.esr_momentum_flush(_p(table), _p(trace), _p(last), V, D, int(step), float(lr), float(momentum), _stream()),
          "esr_momentum_flush")


def spotify_get_embeddings(album_table, artist_table, album_ids, artist_ids):
    """[count, 2F] = concat(album_table[album mod rows], artist_table[artist]) (spotify/models.py:37-51)."""
    lib = _lib.load()
    _req(album_table, torch.float32, "album_table"), _req(artist_table, torch.float32, "artist_table")
    album_ids, artist_ids = _req(album_ids, torch.int32, "album_ids"), _req(artist_ids, torch.int32, "artist_ids")
    count, F = album_ids.numel(), album_table.shape[1]
    out = torch.empty((count, 2 * F), dtype=torch.float32, device=album_table.device)
    l2 = torch.empty(count, dtype=torch.float32, device=album_table.device)
    check(lib.esr_spotify_get_embeddings(_p(album_table), album_table.shape[0], _p(artist_table),
                                         artist_table.shape[0], F, _p(album_ids), _p(artist_ids), count, _p(out),
                                         _p(l2), _stream()), "esr_spotify_get_embeddings")
    return out


def _sp_occurrences(who, album_ids, artist_ids, n, m, o):
    """The kernels read n + m + o ids from both tensors: a shorter one would be read past its end on the device."""
    R = int(n) + int(m) + int(o)
    for t, name in ((album_ids, "album_ids"), (artist_ids, "artist_ids")):
        if isinstance(t, torch.Tensor) and t.numel() != R:
            raise ValueError("%s: %s holds %d entries, n + m + o = %d + %d + %d = %d are required"
                             % (who, name, t.numel(), n, m, o, R))


def spotify_forward(album_table, artist_table, album_ids, artist_ids, n, m, o):
    """SpotifyModel.__call__ (spotify/models.py:53-90) on occurrence ids ordered context, next, neg."""
    _sp_occurrences("spotify_forward", album_ids, artist_ids, n, m, o)
    lib = _lib.load()
    _req(album_table, torch.float32, "album_table"), _req(artist_table, torch.float32, "artist_table")
    album_ids, artist_ids = _req(album_ids, torch.int32, "album_ids"), _req(artist_ids, torch.int32, "artist_ids")
    F, dev = album_table.shape[1], album_table.device
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    pos, neg, cs, ns, gs, l2 = f(m), f(o), f(n, n), f(m, m), f(o, o), f(n + m + o)
    ws = _ws(_ws_bytes("esr_spotify_workspace_bytes", n, m, o, F), dev)
    check(lib.esr_spotify_forward(_p(album_table), album_table.shape[0], _p(artist_table), artist_table.shape[0], F,
                                  _p(album_ids), _p(artist_ids), n, m, o, _p(pos), _p(neg), _p(cs), _p(ns), _p(gs),
                                  _p(l2), _p(ws), ws.numel(), _stream()), "esr_spotify_forward")
    return pos, neg, cs, ns, gs, l2


def spotify_fwd_bwd(album_table, artist_table, album_ids, artist_ids, n, m, o, regularization):
    """loss and per-occurrence gradient rows of train_spotify.py:78-109.
    Returns (loss[1], album_rows[R] (hashed ids), g_album_rows[R, F], g_artist_rows[R, F])."""
    _sp_occurrences("spotify_fwd_bwd", album_ids, artist_ids, n, m, o)
    lib = _lib.load()
    _req(album_table, torch.float32, "album_table"), _req(artist_table, torch.float32, "artist_table")
    album_ids, artist_ids = _req(album_ids, torch.int32, "album_ids"), _req(artist_ids, torch.int32, "artist_ids")
    F, dev, R = album_table.shape[1], album_table.device, n + m + o
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    rows = torch.empty(R, dtype=torch.int32, device=dev)
    ga = torch.empty((R, F), dtype=torch.float32, device=dev)
    gr = torch.empty((R, F), dtype=torch.float32, device=dev)
    ws = _ws(_ws_bytes("esr_spotify_workspace_bytes", n, m, o, F), dev)
    check(lib.esr_spotify_fwd_bwd(_p(album_table), album_table.shape[0], _p(artist_table), artist_table.shape[0], F,
                                  _p(album_ids), _p(artist_ids), n, m, o, float(regularization), _p(loss), _p(rows),
                                  _p(ga), _p(gr), _p(ws), ws.numel(), _stream()), "esr_spotify_fwd_bwd")
    return loss, rows, ga, gr


def spotify_train_step(album_table, album_trace, album_last, artist_table, artist_trace, artist_last, album_ids,
                       artist_ids, n, m, o, regularization, step, lr, momentum):
    """One whole Spotify train step under lazy optax.sgd(lr, momentum) by ONE library call (esr_spotify_train_step): catch
    the playlist's rows up, loss + gradient rows, one sort, the momentum step on the touched rows of both tables.
    Returns loss[1]."""
    _sp_occurrences("spotify_train_step", album_ids, artist_ids, n, m, o)
    lib = _lib.load()
    for t, name in ((album_table, "album_table"), (album_trace, "album_trace"), (artist_table, "artist_table"),
                    (artist_trace, "artist_trace")):
        _req(t, torch.float32, name)
    _req(album_last, torch.int32, "album_last"), _req(artist_last, torch.int32, "artist_last")
    album_ids, artist_ids = _req(album_ids, torch.int32, "album_ids"), _req(artist_ids, torch.int32, "artist_ids")
    F, dev = album_table.shape[1], album_table.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _ws(_ws_bytes("esr_spotify_train_step_workspace_bytes", n, m, o, F), dev)
    check(lib.esr_spotify_train_step(_p(album_table), _p(album_trace), _p(album_last), album_table.shape[0],
                                     _p(artist_table), _p(artist_trace), _p(artist_last), artist_table.shape[0], F,
                                     _p(album_ids), _p(artist_ids), n, m, o, float(regularization), int(step), float(lr),
                                     float(momentum), _p(loss), _p(ws), ws.numel(), _stream()), "esr_spotify_train_step")
    return loss


def spotify_sample_negatives(all_albums, all_artists, seed, step, num_negatives):
    """The negatives of global step `step` (>= 1) drawn on the device (esr_spotify_sample_negatives): Philox4x32-10 keyed by
    the 64-bit `seed`, counter (i >> 2, step, 0, 0), index = (word * (T - 1)) >> 32 -- the last track is never drawn, as in
    train_spotify.py:146; multiply-high is biased by at most (T - 1) / 2^32 relative (5.3e-4 at the reference's corpus).
    all_albums / all_artists: device int32 [T].  Returns (index, album, artist), int32 [num_negatives] each."""
    lib = _lib.load()
    _req(all_albums, torch.int32, "all_albums"), _req(all_artists, torch.int32, "all_artists")
    T, o = all_albums.numel(), int(num_negatives)
    if all_artists.numel() != T:
        raise ValueError("all_albums and all_artists differ in length (%d vs %d)" % (T, all_artists.numel()))
    if T < 2 or o < 1 or int(step) < 1:
        raise ValueError("spotify_sample_negatives: T=%d num_negatives=%d step=%d (T >= 2, num_negatives >= 1, step >= 1)"
                         % (T, o, step))
    out = torch.empty((3, o), dtype=torch.int32, device=all_albums.device)
    check(lib.esr_spotify_sample_negatives(_p(all_albums), _p(all_artists), T, int(seed) & (2 ** 64 - 1), int(step), o,
                                           _p(out[0]), _p(out[1]), _p(out[2]), _stream()), "esr_spotify_sample_negatives")
    return out[0], out[1], out[2]


def spotify_list_starts(n, next_offsets, o):
    """Where esr_spotify_train_steps puts step j's id lists in its workspace (include/esr_hip.h), in int32 units: block j
    = [album ids R_j][artist ids R_j], R_j = n + m_j + o.  next_offsets: the K + 1 host offsets."""
    off = np.asarray(next_offsets, dtype=np.int64)
    j = np.arange(off.size - 1, dtype=np.int64)
    return (2 * (j * (n + o) + off[:-1]) + 63) // 64 * 64 + 64 * j


def spotify_train_steps(album_table, album_trace, album_last, artist_table, artist_trace, artist_last, ctx_album, ctx_artist,
                        next_album, next_artist, next_offsets, next_offsets_dev, all_albums, all_artists, seed, first_step,
                        num_negatives, regularization, lr, momentum, losses=None, neg_index=None, workspace=None):
    """K Spotify train steps under lazy optax.sgd(lr, momentum) by ONE library call (esr_spotify_train_steps): one launch
    draws the negatives of steps first_step .. first_step + K - 1 and assembles every step's id lists, then each step is
    the launch sequence of spotify_train_step.  ctx_album / ctx_artist: device int32 [K, n]; next_album / next_artist:
    device int32, the K next lists packed; next_offsets: host int64 [K + 1] (numpy), next_offsets_dev: its device copy.
    losses (float32 [K]), neg_index (int32 [K, num_negatives]) and workspace (uint8) are outputs the caller may provide.
    Returns losses."""
    lib = _lib.load()
    for t, name in ((album_table, "album_table"), (album_trace, "album_trace"), (artist_table, "artist_table"),
                    (artist_trace, "artist_trace")):
        _req(t, torch.float32, name)
    for t, name in ((album_last, "album_last"), (artist_last, "artist_last"), (ctx_album, "ctx_album"),
                    (ctx_artist, "ctx_artist"), (next_album, "next_album"), (next_artist, "next_artist"),
                    (all_albums, "all_albums"), (all_artists, "all_artists")):
        _req(t, torch.int32, name)
    _req(next_offsets_dev, torch.int64, "next_offsets_dev")
    if ctx_album.dim() != 2 or ctx_album.shape != ctx_artist.shape:
        raise ValueError("ctx_album / ctx_artist must both be [K, n], got %s and %s"
                         % (tuple(ctx_album.shape), tuple(ctx_artist.shape)))
    K, n = ctx_album.shape
    off = np.ascontiguousarray(next_offsets, dtype=np.int64)
    if off.ndim != 1 or off.size != K + 1 or next_offsets_dev.numel() != K + 1:
        raise ValueError("next_offsets / next_offsets_dev must hold K + 1 = %d entries" % (K + 1))
    if K < 1 or off[0] != 0 or (np.diff(off) < 1).any():
        raise ValueError("spotify_train_steps: K >= 1 playlists, next_offsets from 0, every next list non-empty")
    total = int(off[-1])
    if next_album.numel() != total or next_artist.numel() != total:
        raise ValueError("next_album / next_artist hold %d / %d ids, next_offsets[K] = %d"
                         % (next_album.numel(), next_artist.numel(), total))
    T, o = all_albums.numel(), int(num_negatives)
    if all_artists.numel() != T:
        raise ValueError("all_albums and all_artists differ in length (%d vs %d)" % (T, all_artists.numel()))
    if T < 2:
        raise ValueError("spotify_train_steps: a corpus of T=%d tracks (T >= 2: the last track is never drawn)" % T)
    F, dev = album_table.shape[1], album_table.device
    if losses is None:
        losses = torch.empty(K, dtype=torch.float32, device=dev)
    elif _req(losses, torch.float32, "losses").numel() != K:
        raise ValueError("losses must hold K = %d entries" % K)
    if neg_index is not None and _req(neg_index, torch.int32, "neg_index").numel() != K * o:
        raise ValueError("neg_index must hold K * num_negatives = %d entries" % (K * o))
    nbytes = _ws_bytes("esr_spotify_train_steps_workspace_bytes", n, int(np.diff(off).max()), o, F, K, total)
    ws = _ws(nbytes, dev) if workspace is None else _req(workspace, torch.uint8, "workspace")
    check(lib.esr_spotify_train_steps(_p(album_table), _p(album_trace), _p(album_last), album_table.shape[0],
                                      _p(artist_table), _p(artist_trace), _p(artist_last), artist_table.shape[0], F, n, o, K,
                                      _p(ctx_album), _p(ctx_artist), _p(next_album), _p(next_artist), off.ctypes.data,
                                      _p(next_offsets_dev), _p(all_albums), _p(all_artists), T, int(seed) & (2 ** 64 - 1),
                                      int(first_step), float(regularization), float(lr), float(momentum), _p(losses),
                                      _p(neg_index), _p(ws), ws.numel(), _stream()), "esr_spotify_train_steps")
    return losses


def spotify_affinity_all(album_table, artist_table, ctx_album, ctx_artist, all_albums, all_artists):
    """Affinity [T] of every track to the context (train_spotify.py:113-119, result[1])."""
    lib = _lib.load()
    _req(album_table, torch.float32, "album_table"), _req(artist_table, torch.float32, "artist_table")
    for t, name in ((ctx_album, "ctx_album"), (ctx_artist, "ctx_artist"), (all_albums, "all_albums"),
                    (all_artists, "all_artists")):
        _req(t, torch.int32, name)
    T = all_albums.numel()
    out = torch.empty(T, dtype=torch.float32, device=album_table.device)
    check(lib.esr_spotify_affinity_all(_p(album_table), album_table.shape[0], _p(artist_table), artist_table.shape[0],
                                       album_table.shape[1], _p(ctx_album), _p(ctx_artist), ctx_album.numel(),
                                       _p(all_albums), _p(all_artists), T, _p(out), _stream()),
          "esr_spotify_affinity_all")
    return out


def spotify_topk_batch(album_table, artist_table, ctx_album, ctx_artist, all_albums, all_artists, k):
    """top_k(affinity, k) over every track for P playlists at once (train_spotify.py:113-120 over the eval loop of
    :270-281): ctx_album / ctx_artist [P, n] -> (scores [P, k] f32, indices [P, k] int32), best first, ties to the
    lower track index.  Row p equals what spotify_affinity_all + a top-k give playlist p, bit for bit."""
    lib = _lib.load()
    _req(album_table, torch.float32, "album_table"), _req(artist_table, torch.float32, "artist_table")
    for t, name in ((ctx_album, "ctx_album"), (ctx_artist, "ctx_artist"), (all_albums, "all_albums"),
                    (all_artists, "all_artists")):
        _req(t, torch.int32, name)
    if album_table.dim() != 2 or artist_table.dim() != 2 or album_table.shape[1] != artist_table.shape[1]:
        raise ValueError("album_table / artist_table must be [rows, F] of one width F")
    if ctx_album.dim() != 2 or ctx_album.shape != ctx_artist.shape:
        raise ValueError("ctx_album / ctx_artist must both be [P, n], got %s and %s"
                         % (tuple(ctx_album.shape), tuple(ctx_artist.shape)))
    P, n = ctx_album.shape
    T = all_albums.numel()
    if all_artists.numel() != T:
        raise ValueError("all_albums and all_artists differ in length (%d vs %d)" % (T, all_artists.numel()))
    F = album_table.shape[1]
    if not (P >= 1 and 1 <= n <= 32 and 1 <= F and 2 * F <= 256 and 1 <= k <= min(T, 1024)):
        raise ValueError("spotify_topk_batch: P=%d n=%d F=%d T=%d k=%d (P >= 1, 1 <= n <= 32, 2F <= 256, "
                         "1 <= k <= min(T, 1024))" % (P, n, F, T, k))
    dev = album_table.device
    scores = torch.empty((P, k), dtype=torch.float32, device=dev)
    indices = torch.empty((P, k), dtype=torch.int32, device=dev)
    # (not through _ws_bytes' cache: the chunk plan reads ESR_SPOTIFY_EVAL_CHUNK at every call)
    ws = _ws(lib.esr_spotify_topk_batch_workspace_bytes(P, n, T, F, k), dev)
    check(lib.esr_spotify_topk_batch(_p(album_table), album_table.shape[0], _p(artist_table), artist_table.shape[0], F,
                                     _p(ctx_album), _p(ctx_artist), P, n, _p(all_albums), _p(all_artists), T, int(k),
                                     _p(scores), _p(indices), _p(ws), ws.numel(), _stream()),
          "esr_spotify_topk_batch")
    return scores, indices


def rows_to_dense(V, D, sorted_ids, perm, grad_rows, out=None):
    """The dense [V, D] gradient (zero-filled, segment sums scattered) the reference's autodiff yields."""
    lib = _lib.load()
    _req(grad_rows, torch.float32, "grad_rows")
    if out is None:
        out = torch.empty((V, D), dtype=torch.float32, device=grad_rows.device)
    n = sorted_ids.numel()
    check(lib.esr_rows_to_dense(_p(out), V, D, _p(sorted_ids), _p(perm), n, _p(grad_rows), _stream()),
          "esr_rows_to_dense")
    return out


def dense_adam(param, mu, nu, grad, lr, step, b1=0.9, b2=0.999, eps=1e-8):
    """In-place optax.adam on every element; `step` is the 1-based count after this update."""
    lib = _lib.load()
    for name, t in (("param", param), ("mu", mu), ("nu", nu), ("grad", grad)):
        _req(t, torch.float32, name)
    check(lib.esr_dense_adam(_p(param), _p(mu), _p(nu), _p(grad), param.numel(), float(lr), float(b1), float(b2),
                             float(eps), int(step), _stream()), "esr_dense_adam")


ADAM_EXACT_STEPS = 8  # include/esr_hip.h ESR_ADAM_EXACT_STEPS: lazy Adam replays gaps up to this long bit-exactly


def _adam_tables(who, tables, mus, nus, lasts, row_offsets):
    """One or two lazily stepped Adam tables of one launch: (D, pointers of tables, mus, nus, lasts, row offsets)"""
    nt = len(tables)
    if not 1 <= nt <= 2 or not (len(mus) == len(nus) == len(lasts) == nt) or len(row_offsets) != nt + 1:
        raise ValueError("%s takes one or two tables" % who)
    for t, m, v, l in zip(tables, mus, nus, lasts):
        _adam_table(t, m, v, l, who)
    _, D, tp, mp, vp, ro = _fused_tables(tables, row_offsets, torch.float32, mu=mus, nu=nus)
    return D, tp, mp, vp, ptr_array(lasts), ro


def _adam_table(table, mu, nu, last, what):
    _req(table, torch.float32, what + " table")
    _req(mu, torch.float32, what + " mu")
    _req(nu, torch.float32, what + " nu")
    _req(last, torch.int32, what + " last")
    if table.dim() != 2 or mu.shape != table.shape or nu.shape != table.shape or tuple(last.shape) != (table.shape[0],):
        raise ValueError("%s: table, mu, nu must be the same [V, D] and last [V]" % what)


def adam_catchup_rows(tables, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """Lazy optax.adam: bring rows up to step - 1 before step `step` reads them.  tables = one or two tuples
    (table, mu, nu, last, ids, modulus): the rows ids % modulus (modulus 0: ids) of that table; one launch."""
    lib = _lib.load()
    if not 1 <= len(tables) <= 2:
        raise ValueError("adam_catchup_rows takes one or two tables")
    args = []
    for k, (table, mu, nu, last, ids, modulus) in enumerate(tables):
        _adam_table(table, mu, nu, last, "adam_catchup_rows")
        _req(ids, torch.int32, "ids")
        args += [_p(table), _p(mu), _p(nu), _p(last), table.shape[0], table.shape[1], _p(ids), ids.numel(), int(modulus)]
    if len(tables) == 1:
        args += [0, 0, 0, 0, 0, 0, 0, 0, 0]
    check(lib.esr_adam_catchup_rows2(*args, int(step), float(lr), float(b1), float(b2), float(eps), _stream()),
          "esr_adam_catchup_rows2")


def sparse_adam_step_lazy(tables, mus, nus, lasts, row_offsets, sorted_vids, perm, grad_rows, lr, step, b1=0.9,
                          b2=0.999, eps=1e-8):
    """Lazy optax.adam step `step` on the touched rows of one or two same-width tables (virtual rows row_offsets[t] + id,
    sorted by segment_sort / segment_sort_multi).  Rows are caught up from their `last` first and marked `step`."""
    lib = _lib.load()
    D, tp, mp, vp, lp, ro = _adam_tables("sparse_adam_step_lazy", tables, mus, nus, lasts, row_offsets)
    _req(grad_rows, torch.float32, "grad_rows")
    check(lib.esr_sparse_adam_step_lazy(tp, mp, vp, lp, ro, len(tables), D, _p(sorted_vids), _p(perm), sorted_vids.numel(),
                                        _p(grad_rows), float(lr), float(b1), float(b2), float(eps), int(step), _stream()),
          "esr_sparse_adam_step_lazy")


def adam_catchup_gather(tables, mus, nus, lasts, row_offsets, sorted_rows, perm, step, lr, b1=0.9, b2=0.999, eps=1e-8,
                        out=None, serve=True):
    """Lazy optax.adam, owner side of a row-sharded lookup: the rows sorted_rows (virtual rows of one or two same-width
    tables, sorted by segment_sort, perm its permutation) brought up to step - 1 and served: returns out [n, D] with
    out[perm[j]] = the caught-up row sorted_rows[j] -- what adam_catchup_rows followed by gather_rows_multi gives, bit for
    bit, in one pass.  serve=False: catch up only (returns None)."""
    lib = _lib.load()
    D, tp, mp, vp, lp, ro = _adam_tables("adam_catchup_gather", tables, mus, nus, lasts, row_offsets)
    _req(sorted_rows, torch.int32, "sorted_rows")
    n = sorted_rows.numel()
    if serve:
        _req(perm, torch.int32, "perm")
        if perm.numel() != n:
            raise ValueError("adam_catchup_gather: sorted_rows and perm differ in length")
        if out is None:
            out = torch.empty((n, D), dtype=torch.float32, device=tables[0].device)
        _req(out, torch.float32, "out")
        if tuple(out.shape) != (n, D):
            raise ValueError("adam_catchup_gather: out must be [%d, %d], got %s" % (n, D, tuple(out.shape)))
    check(lib.esr_adam_catchup_gather(tp, mp, vp, lp, ro, len(tables), D, _p(sorted_rows),
                                      _p(perm) if serve else None, n, _p(out) if serve else None, int(step), float(lr),
                                      float(b1), float(b2), float(eps), _stream()), "esr_adam_catchup_gather")
    return out if serve else None


def adam_flush(table, mu, nu, last, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """Lazy optax.adam: every row with last < step brought up to `step` (p, mu and nu); last = step afterwards."""
    lib = _lib.load()
    _adam_table(table, mu, nu, last, "adam_flush")
    check(lib.esr_adam_flush(_p(table), _p(mu), _p(nu), _p(last), table.shape[0], table.shape[1], int(step), float(lr),
                             float(b1), float(b2), float(eps), _stream()), "esr_adam_flush")


# ---------------------------------------------------------------------------------------------
def score_all(emb, token):
    """scores[v, t] = emb[v] . emb[token[t]]  -> [V, T]."""
    lib = _lib.load()
    _req(emb, torch.float32, "emb"), _req(token, torch.int32, "token")
    V, D = emb.shape
    T = token.numel()
    scores = torch.empty((V, T), dtype=torch.float32, device=emb.device)
    check(lib.esr_score_all(_p(emb), V, D, _p(token), T, _p(scores), _stream()), "esr_score_all")
    return scores


def argsort_columns(scores):
    """Stable ascending argsort of every column of scores [V, T] -> int32 [V, T]."""
    lib = _lib.load()
    _req(scores, torch.float32, "scores")
    V, T = scores.shape
    indices = torch.empty((V, T), dtype=torch.int32, device=scores.device)
    ws = _ws(_ws_bytes("esr_argsort_columns_workspace_bytes", V, T), scores.device)
    check(lib.esr_argsort_columns(_p(scores), V, T, _p(indices), _p(ws), ws.numel(), _stream()),
          "esr_argsort_columns")
    return indices


def score_topk(queries, candidates, k):
    """Top-k of queries @ candidates^T per query (descending, ties -> lower index)."""
    lib = _lib.load()
    _req(queries, torch.float32, "queries"), _req(candidates, torch.float32, "candidates")
    nq, D = queries.shape
    N = candidates.shape[0]
    out_s = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
    out_i = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
    ws = _ws(_ws_bytes("esr_score_topk_workspace_bytes", nq, N, k), queries.device)
    check(lib.esr_score_topk(_p(queries), _p(candidates), nq, N, D, k, _p(out_s), _p(out_i), _p(ws), ws.numel(),
                             _stream()), "esr_score_topk")
    return out_s, out_i


_RETRIEVE_MODES = {"bf16x3": _lib.RETRIEVE_EXACT, "f16x2": _lib.RETRIEVE_F16X2, "bf16": _lib.RETRIEVE_BF16,
                   "f16r": _lib.RETRIEVE_F16R}


def _retrieve_mode(mode):
    """"exact" / "f32": the exact-split path -- every f32 operand as three bf16 planes (24 significand bits, whatever the
    dynamic range of the matrix), six MFMA terms per product.  "f16x2" must be asked for by name: two fp16 planes of
    x * 2^e with ONE exponent per matrix (three MFMA terms, 1.6x faster at C5): f32-grade while the matrix's elements
    lie within ~2^16 of its largest one, absolute (not relative) error below that -- near-tie orderings can then differ
    from the f32 brute force.  (ESR_RETRIEVE_EXACT=f16x2 restores round 2's mapping.)"""
    if mode in ("exact", "f32"):
        mode = os.environ.get("ESR_RETRIEVE_EXACT", "bf16x3")
    if mode not in _RETRIEVE_MODES:
        raise ValueError("retrieval mode must be exact / f32 / f16x2 / f16r / bf16x3 / bf16, got %r" % (mode,))
    return _RETRIEVE_MODES[mode]


class PreparedCorpus:
    """What retrieve_prepare made of a candidate matrix: the buffer esr_retrieve_topk_prepared reads, and what it was made
    for (mode, shape, the matrix's storage and its version counter) so that a call cannot be handed another corpus's or
    another mode's planes, nor planes older than the matrix.  The matrix itself is kept: while it lives, no other tensor
    gets its address; an in-place update (a training step) bumps its version, and the stale planes and statistics are
    refused rather than used.  (An inference tensor keeps no version counter: for one, only the address is checked.)"""
    __slots__ = ("blob", "mode", "N", "D", "data_ptr", "candidates", "version")

    def __init__(self, blob, mode, candidates):
        self.blob, self.mode, self.candidates = blob, mode, candidates
        self.N, self.D = candidates.shape
        self.data_ptr, self.version = candidates.data_ptr(), _version_of(candidates)

    def matches(self, candidates, mode):
        return (self.mode, self.N, self.D, self.data_ptr, self.version) == \
            (mode, candidates.shape[0], candidates.shape[1], candidates.data_ptr(), _version_of(candidates))


def _version_of(t):
    return None if t.is_inference() else t._version


def retrieve_prepare(candidates, mode="f16r"):
    """The per-corpus half of retrieve_topk done once (esr_retrieve_prepare): the candidates' scaling statistics and their
    planes in the mode's format, to pass as retrieve_topk(..., prepared=...) for as long as `candidates` is unchanged (a
    product table that serves many scene batches: pinterest/make_recommendations.py:123-132)."""
    lib = _lib.load()
    _req(candidates, torch.float32, "candidates")
    N, D = candidates.shape
    m = _retrieve_mode(mode)
    nbytes = lib.esr_retrieve_prepared_bytes(N, D, m)
    if nbytes == 0:
        raise ValueError("retrieve_prepare: bad shape %s / mode %r" % (tuple(candidates.shape), mode))
    blob = _aligned_bytes(nbytes, candidates.device)
    check(lib.esr_retrieve_prepare(_p(candidates), N, D, m, _p(blob), blob.numel(), _stream()), "esr_retrieve_prepare")
    return PreparedCorpus(blob, m, candidates)


def retrieve_topk(queries, candidates, k, mode="exact", index_base=0, index_step=1, prepared=None):
    """Batched brute-force top-k of queries @ candidates^T (descending, ties -> lower index) on MFMA.
    mode "exact" = "bf16x3": three exact bf16 planes per operand (exact products in f32 accumulation order);
    "f16x2": two scaled fp16 planes (f32-grade within a 2^16 dynamic range per matrix, 1.6x faster); "f16r": one scaled
    fp16 plane as a filter with a proven error band, its survivors re-scored in f32 -- the exact top-k of the f32 scores
    at a third of f16x2's matrix work (include/esr_hip.h ESR_RETRIEVE_F16R); "bf16": one plane (approximate).
    Reported indices are index_base + n * index_step for local candidate row n.
    prepared: retrieve_prepare(candidates, mode) -- the candidates' statistics and planes made once."""
    lib = _lib.load()
    _req(queries, torch.float32, "queries"), _req(candidates, torch.float32, "candidates")
    nq, D = queries.shape
    N = candidates.shape[0]
    m = _retrieve_mode(mode)
    out_s = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
    out_i = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
    ws = _ws(_ws_bytes("esr_retrieve_workspace_bytes", nq, N, D, k, m), queries.device)
    if prepared is not None:
        if not isinstance(prepared, PreparedCorpus) or not prepared.matches(candidates, m):
            raise ValueError("prepared must be retrieve_prepare(candidates, mode) of THIS candidate matrix and mode, "
                             "made after its last in-place update")
        check(lib.esr_retrieve_topk_prepared(_p(queries), _p(candidates), _p(prepared.blob), nq, N, D, k, m, index_base,
                                             index_step, _p(out_s), _p(out_i), _p(ws), ws.numel(), _stream()),
              "esr_retrieve_topk_prepared")
        return out_s, out_i
    check(lib.esr_retrieve_topk(_p(queries), _p(candidates), nq, N, D, k, m, index_base, index_step, _p(out_s),
                                _p(out_i), _p(ws), ws.numel(), _stream()), "esr_retrieve_topk")
    return out_s, out_i


def rescore_candidates(queries, candidates, indices, index_base=0, index_step=1):
    """scores[q, j] = queries[q] . candidates[(indices[q, j] - index_base) // index_step] in f32."""
    lib = _lib.load()
    _req(queries, torch.float32, "queries"), _req(candidates, torch.float32, "candidates")
    indices = _req(indices, torch.int32, "indices")
    nq, D = queries.shape
    out = torch.empty(indices.shape, dtype=torch.float32, device=queries.device)
    check(lib.esr_rescore_candidates(_p(queries), _p(candidates), nq, candidates.shape[0], D, _p(indices),
                                     indices.shape[1], index_base, index_step, _p(out), _stream()),
          "esr_rescore_candidates")
    return out


def topk_merge(scores, indices, k):
    """Top-k of per-query (score, index) lists [nq, n] (descending, ties -> lower index)."""
    lib = _lib.load()
    scores = _req(scores, torch.float32, "scores")
    indices = _req(indices, torch.int32, "indices")
    nq, n = scores.shape
    out_s = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((nq, k), dtype=torch.int32, device=scores.device)
    check(lib.esr_topk_merge(_p(scores), _p(indices), nq, n, k, _p(out_s), _p(out_i), _stream()), "esr_topk_merge")
    return out_s, out_i


def inbatch_towers_fwd_bwd(query_table, cand_table, query_ids, cand_ids, scale, regularization, batch_size,
                           grad_positions=None, precision="auto"):
    """In-batch softmax step head straight from the tower tables (no materialised Q / C): rows query_table[query_ids],
    cand_table[cand_ids]; tables f32 or bf16 [V, 128], B % 128 == 0.  Returns (loss[1], lse[B], gQ, gC) like
    inbatch_softmax_fwd_bwd.  precision: "auto" / "f16x2" / "bf16x3" (see inbatch_split_path; bf16 tables always take
    the bf16x3 kernels, where they are one-plane).  grad_positions = (gq_rows, gc_rows) int32 [B] each: the gradient
    rows are scattered into ONE [2B, 128] buffer at those rows instead (returned as gQ, with gC = None)."""
    lib = _lib.load()
    dt = _table_dtype(query_table, "query_table")
    if _table_dtype(cand_table, "cand_table") != dt:
        raise TypeError("both tower tables must have the same dtype")
    query_ids, cand_ids = _req(query_ids, torch.int32, "query_ids"), _req(cand_ids, torch.int32, "cand_ids")
    B, D, dev = query_ids.numel(), query_table.shape[1], query_table.device
    path = inbatch_split_path(precision, B, D, bf16_tables=query_table.dtype == torch.bfloat16)
    if path is None:
        raise ValueError("inbatch_towers_fwd_bwd needs D <= 128 (a multiple of 4) and B %% 128 == 0 (got B=%d, D=%d) and a split precision"
                         % (B, D))
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    lse = torch.empty(B, dtype=torch.float32, device=dev)
    gQC = torch.empty((2 * B, D), dtype=torch.float32, device=dev)
    if path == "f16x2":
        ws = _ws(_ws_bytes("esr_inbatch2h_workspace_bytes", B, D), dev)
        fn, name = lib.esr_inbatch_towers_fwd_bwd_f16x2, "esr_inbatch_towers_fwd_bwd_f16x2"
    else:
        ws = _ws(_ws_bytes("esr_inbatch3_workspace_bytes", B, D), dev)
        fn, name = lib.esr_inbatch_towers_fwd_bwd_bf16x3, "esr_inbatch_towers_fwd_bwd_bf16x3"
    if grad_positions is not None:
        gqr, gcr = _req(grad_positions[0], torch.int32, "gq_rows"), _req(grad_positions[1], torch.int32, "gc_rows")
        gq_ptr = gc_ptr = _p(gQC)
    else:
        gqr = gcr = None
        gq_ptr, gc_ptr = _p(gQC[:B]), _p(gQC[B:])
    check(fn(_p(query_table), query_table.shape[0], _p(cand_table), cand_table.shape[0], dt, D, _p(query_ids),
             _p(cand_ids), _p(gqr), _p(gcr), B, float(scale), float(regularization), float(batch_size), _p(loss),
             _p(lse), gq_ptr, gc_ptr, _p(ws), ws.numel(), _stream()), name)
    if grad_positions is not None:
        return loss, lse, gQC, None
    return loss, lse, gQC[:B], gQC[B:]


def inbatch_train_step(query_table, query_accum, cand_table, cand_accum, query_ids, cand_ids, scale, regularization,
                       batch_size, lr, eps=1e-7, presorted=None, long_runs=-1, side_stream=None, want_lse=False):
    """One whole in-batch training step of the two towers (esr_inbatch_train_step_f16x2): gather + fp16 x 2 score passes +
    row-sparse Adagrad on both towers, in place.  presorted = (sorted virtual ids, perm) of [query_ids ; Vq + cand_ids]
    (segment_sort_multi / segment_sort_batched), else the list is sorted here; long_runs: 0 when long_run_hint said no id
    occurs more than 32 times.  side_stream (a torch.cuda.Stream of the same device): merge<Q> and the query tower's
    update run on it beside pass C (bit-identical results).  Returns loss[1] (and lse[B] with want_lse)."""
    lib = _lib.load()
    dt = _table_dtype(query_table, "query_table")
    if _table_dtype(cand_table, "cand_table") != dt:
        raise TypeError("both tower tables must have the same dtype")
    _req(query_accum, torch.float32, "query_accum"), _req(cand_accum, torch.float32, "cand_accum")
    query_ids, cand_ids = _req(query_ids, torch.int32, "query_ids"), _req(cand_ids, torch.int32, "cand_ids")
    B, D, dev = query_ids.numel(), query_table.shape[1], query_table.device
    if cand_ids.numel() != B or cand_table.shape[1] != D:
        raise ValueError("id counts / tower widths differ")
    if query_accum.shape != query_table.shape or cand_accum.shape != cand_table.shape:
        raise ValueError("accumulator shapes do not match their towers")
    if not (D % 4 == 0 and 0 < D <= 128 and B % 128 == 0 and 0 < B <= INBATCH_F16X2_MAX_B):
        raise ValueError("inbatch_train_step needs D <= 128 (a multiple of 4), B %% 128 == 0 and B <= %d (got B=%d, D=%d)"
                         % (INBATCH_F16X2_MAX_B, B, D))
    sid = perm = None
    if presorted is not None:
        sid, perm = _req(presorted[0], torch.int32, "sorted_ids"), _req(presorted[1], torch.int32, "perm")
        if sid.numel() != 2 * B or perm.numel() != 2 * B:
            raise ValueError("presorted ids / perm must have 2 B entries")
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    lse = torch.empty(B, dtype=torch.float32, device=dev) if want_lse else None
    ws = _ws(_ws_bytes("esr_inbatch_train_step_workspace_bytes", B, D), dev)
    side = side_stream.cuda_stream if side_stream is not None else None
    check(lib.esr_inbatch_train_step_f16x2(_p(query_table), _p(query_accum), query_table.shape[0], _p(cand_table),
                                           _p(cand_accum), cand_table.shape[0], dt, D, _p(query_ids), _p(cand_ids), B,
                                           float(scale), float(regularization), float(batch_size), float(lr), float(eps),
                                           _p(sid), _p(perm), int(long_runs), _p(loss), _p(lse), _p(ws), ws.numel(),
                                           _stream(), side), "esr_inbatch_train_step_f16x2")
    if side_stream is not None:
        ws.record_stream(side_stream)  # (the call joined the streams; this only tells torch's allocator who used the block)
    return (loss, lse) if want_lse else loss


def sorted_membership(cur, seq, sentinel):
    """flags uint8 [L, n]: cur[l, j] != sentinel and cur[l, j] occurs in the ascending row seq[l] (esr_sorted_membership)."""
    lib = _lib.load()
    cur, seq = _req(cur, torch.int32, "cur"), _req(seq, torch.int32, "seq")
    L, n = cur.shape
    flags = torch.empty((L, n), dtype=torch.uint8, device=cur.device)
    check(lib.esr_sorted_membership(_p(cur), n, _p(seq), seq.shape[1], L, int(sentinel), _p(flags), _stream()),
          "esr_sorted_membership")
    return flags


def flagged_first(flags, values, slice_len, counts_out):
    """Stable partition of every row of `values` [L, n] (None: the positions 0 .. n - 1) by flags uint8 [L, n]: returns
    int32 [L, n] whose rows START with the flagged entries in order (the rest is unspecified); counts_out int64 [G, L]
    (any strides) receives, per row, the flagged entries inside each of G consecutive slices of lengths slice_len int64
    [L, G] (esr_flagged_first)."""
    lib = _lib.load()
    flags = _req(flags, torch.uint8, "flags")
    L, n = flags.shape
    slice_len = _req(slice_len, torch.int64, "slice_len")
    G = slice_len.shape[1]
    if values is not None:
        values = _req(values, torch.int32, "values")
    if counts_out.dtype != torch.int64 or tuple(counts_out.shape) != (G, L):
        raise ValueError("counts_out must be an int64 [G, L] view")
    out = torch.empty((L, n), dtype=torch.int32, device=flags.device)
    ws = _ws(_ws_bytes("esr_flagged_first_workspace_bytes", n, L), flags.device)
    check(lib.esr_flagged_first(_p(flags), _p(values), n, L, _p(slice_len), G, _p(out), counts_out.data_ptr(),
                                counts_out.stride(1), counts_out.stride(0), _p(ws), ws.numel(), _stream()),
          "esr_flagged_first")
    return out


def run_offsets(sorted_ids, nvalues, want_max=False):
    """int32 [nvalues + 1]: the first position of each value in the ascending int32 list (esr_run_offsets); with want_max
    also the longest run as an int32 [1] device tensor."""
    lib = _lib.load()
    sorted_ids = _req(sorted_ids, torch.int32, "sorted_ids")
    off = torch.empty(nvalues + 1, dtype=torch.int32, device=sorted_ids.device)
    mx = torch.empty(1, dtype=torch.int32, device=sorted_ids.device) if want_max else None
    check(lib.esr_run_offsets(_p(sorted_ids), sorted_ids.numel(), int(nvalues), _p(off), _p(mx), _stream()), "esr_run_offsets")
    return (off, mx) if want_max else off


def ivf_centroids(sums, list_off=None, train=None, fallback_rows=None):
    """Unit-length centroids from per-list sums [nlist, D]; a list without members (list_off) takes training row
    fallback_rows[v] instead (esr_ivf_centroids)."""
    lib = _lib.load()
    sums = _req(sums, torch.float32, "sums")
    nlist, D = sums.shape
    out = torch.empty_like(sums)
    check(lib.esr_ivf_centroids(_p(sums), _p(list_off), _p(train), _p(fallback_rows), nlist, D, _p(out), _stream()),
          "esr_ivf_centroids")
    return out


def recall_at_k(approx_indices, exact_indices):
    """hits / (Q * ke): the fraction of exact_indices [Q, ke] that also occur in the same row of approx_indices [Q, ka]
    (esr_recall_at_k).  Synchronises to read the one counter back."""
    lib = _lib.load()
    a = approx_indices if approx_indices.dtype == torch.int32 else approx_indices.to(torch.int32)
    e = exact_indices if exact_indices.dtype == torch.int32 else exact_indices.to(torch.int32)
    a, e = _req(a.contiguous(), torch.int32, "approx_indices"), _req(e.contiguous(), torch.int32, "exact_indices")
    if a.dim() != 2 or e.dim() != 2 or a.shape[0] != e.shape[0]:
        raise ValueError("approx_indices [Q, ka] and exact_indices [Q, ke] must have the same number of rows")
    hits = torch.empty(1, dtype=torch.int64, device=a.device)
    check(lib.esr_recall_at_k(_p(a), a.shape[0], a.shape[1], _p(e), e.shape[1], _p(hits), _stream()), "esr_recall_at_k")
    return float(int(hits.item())) / max(1, e.numel())


def bucket_ids_by_owner_batched(id_lists, world, offsets):
    """bucket_ids_by_owner for the lists of several coming batches in one launch pair (esr_bucket_ids_by_owner_batched).
    id_lists: per batch, the int32 segments of its virtual list [ids_k + offsets[k]] (same lengths in every batch).
    Returns (local_rows [L, n], perm [L, n], counts [L, world] int64, inverse [L, n])."""
    lib = _lib.load()
    nb, nseg = len(id_lists), len(id_lists[0])
    ptrs, cnt, off, _, n, dev = _id_segments_batched(id_lists, offsets)
    local_rows = torch.empty((nb, n), dtype=torch.int32, device=dev)
    perm = torch.empty((nb, n), dtype=torch.int32, device=dev)
    inverse = torch.empty((nb, n), dtype=torch.int32, device=dev)
    counts = torch.empty((nb, world), dtype=torch.int64, device=dev)
    ws = _ws(_ws_bytes("esr_bucket_batched_workspace_bytes", n, nb), dev)
    check(lib.esr_bucket_ids_by_owner_batched(ptrs, cnt, off, nseg, nb, int(world), _p(local_rows), _p(perm), _p(inverse),
                                              _p(counts), _p(ws), ws.numel(), _stream()),
          "esr_bucket_ids_by_owner_batched")
    return local_rows, perm, counts, inverse


def segment_sort_batched(id_lists, offsets, num_rows, out=None):
    """The occurrence lists of several coming batches sorted in one launch sequence (esr_segment_sort_ids_batched).
    id_lists: per batch, the int32 segments of its virtual list [ids_k + offsets[k]] (same lengths in every batch).
    Returns (sorted_ids, perm), each [len(id_lists), n]: row b is what segment_sort / the multi-segment sort gives for
    batch b alone.  out = (sorted_ids, perm, workspace) to reuse buffers."""
    lib = _lib.load()
    nb, nseg = len(id_lists), len(id_lists[0])
    ptrs, cnt, off, _, n, dev = _id_segments_batched(id_lists, offsets)
    if out is None:
        sorted_ids = torch.empty((nb, n), dtype=torch.int32, device=dev)
        perm = torch.empty((nb, n), dtype=torch.int32, device=dev)
        ws = _ws(_ws_bytes("esr_segment_sort_batched_workspace_bytes", n, nb), dev)
    else:
        sorted_ids, perm, ws = out
    check(lib.esr_segment_sort_ids_batched(ptrs, cnt, off, nseg, nb, int(num_rows), _p(sorted_ids), _p(perm), _p(ws),
                                           ws.numel(), _stream()), "esr_segment_sort_ids_batched")
    return sorted_ids, perm


def bucket_ids_by_owner(ids, world, want_inverse=False, offsets=None, counts_out=None):
    """Stable bucket by owner = id % world.  Returns (local_rows, perm, counts[world] int64 on device) and, with
    want_inverse, also inverse with inverse[perm[k]] = k.  `ids` may be a list of int32 tensors with `offsets`: the
    virtual list [ids_0 + offsets[0] ; ids_1 + offsets[1] ; ...] is bucketed in place (no concatenated copy).
    `counts_out` (contiguous int64 [world] on the device) receives the counts instead of a fresh tensor."""
    lib = _lib.load()
    segs = list(ids) if isinstance(ids, (list, tuple)) else None
    if segs is None:
        ids = _req(ids, torch.int32, "ids")
        n, dev = ids.numel(), ids.device
    else:
        ptrs, cnt, off, _, n, dev = _id_segments(segs, offsets if offsets is not None else [0] * len(segs))
    local_rows = torch.empty(n, dtype=torch.int32, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    inverse = torch.empty(n, dtype=torch.int32, device=dev) if want_inverse else None
    if counts_out is None:
        counts = torch.empty(world, dtype=torch.int64, device=dev)
    else:
        counts = _req(counts_out, torch.int64, "counts_out")
        if counts.numel() != world:
            raise ValueError("counts_out must hold %d int64" % world)
    ws = _ws(_ws_bytes("esr_bucket_workspace_bytes", n), dev)
    if segs is None:
        check(lib.esr_bucket_ids_by_owner(_p(ids), n, world, _p(local_rows), _p(perm), _p(inverse), _p(counts), _p(ws),
                                          ws.numel(), _stream()), "esr_bucket_ids_by_owner")
    else:
        check(lib.esr_bucket_ids_by_owner_multi(ptrs, cnt, off, len(segs), world, _p(local_rows), _p(perm), _p(inverse),
                                                _p(counts), _p(ws), ws.numel(), _stream()),
              "esr_bucket_ids_by_owner_multi")
    if want_inverse:
        return local_rows, perm, counts, inverse
    return local_rows, perm, counts


# ---- a row-sharded step's exchange halves, one library call each (esr_shard_step.hip) ----------------------------------
def sharded_lookup(comm, world, tables_c, loff_c, ntables, dtype, D, asked_rows, asked_c, ask_c, served, back):
    """esr_sharded_lookup: gather the rows asked of this rank + the rows exchange, on the current stream.  `comm`: the
    DirectExchange communicator (ctypes.c_void_p) or None at world 1; served may be None at world 1."""
    lib = _lib.load()
    check(lib.esr_sharded_lookup(comm, world, tables_c, loff_c, ntables, dtype, D, _p(asked_rows), asked_c, ask_c,
                                 _p(served) if served is not None else None, _p(back), _stream()),
          "esr_sharded_lookup")
    return back


def sharded_update(comm, world, tables_c, accums_c, loff_c, ntables, dtype, D, grad_rows, sorted_uidx, occ_perm, summed,
                   ask_c, asked_c, grad_dtype, send_bf16, recv_raw, recv_grads, owner_sorted, owner_perm, lr, eps=1e-7,
                   long_runs=-1):
    """esr_sharded_update: [per-distinct-row sum ->] gradient rows to their owners -> the owner's fused segment-reduce +
    Adagrad, on the current stream."""
    lib = _lib.load()
    q = lambda t: _p(t) if t is not None else None  # noqa: E731
    check(lib.esr_sharded_update(comm, world, tables_c, accums_c, loff_c, ntables, dtype, D, _p(grad_rows),
                                 int(grad_rows.shape[0]), q(sorted_uidx), q(occ_perm), q(summed), ask_c, asked_c,
                                 grad_dtype, q(send_bf16), q(recv_raw), q(recv_grads), q(owner_sorted), q(owner_perm),
                                 float(lr), float(eps), int(long_runs), _stream()), "esr_sharded_update")


def shard_group_struct(comm, world, tables_c, accums_c, loff_c, ntables, dtype, D, grad_dtype):
    """esr_shard_group_t over the host arrays of ptr_array / i64_array (the caller keeps them -- and the tensors -- alive)."""
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    comm = getattr(comm, "value", comm)
    return _lib.ShardGroupStruct(comm, world, cast(tables_c), cast(accums_c), cast(loff_c), ntables, dtype, D, grad_dtype)


def routing_plan_struct(asked_rows, asked_c, ask_c, index, sorted_uidx, occ_perm, owner_sorted, owner_perm, long_runs=-1):
    """esr_routing_plan_t of one batch (device tensors + the host count arrays; the caller keeps them alive)."""
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    q = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    return _lib.RoutingPlanStruct(q(asked_rows), cast(asked_c), cast(ask_c), q(index), q(sorted_uidx), q(occ_perm),
                                  q(owner_sorted), q(owner_perm), int(long_runs))


def step_overlap_struct(backs, ready, stale, next_plan_s, next_backs, next_serveds, comm2, side_stream):
    """esr_step_overlap_t of one overlapped step (include/esr_hip.h).  backs: this batch's rows per group as the previous
    call fetched them (None: look up in line) with `ready`, that call's next_ready; stale = (rows, asked host array, pos, ask
    host array) of esrecsys_amd.sharded.StaleRows; next_*: the coming batch's plan struct and its buffers per group (None:
    last step); side_stream: a torch.cuda.Stream.  The caller keeps every tensor / array alive until the NEXT call."""
    ov = _lib.StepOverlapStruct()
    q = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    for i, b in enumerate(backs or ()):
        ov.back[i] = b.data_ptr()
    ov.ready = ready
    if backs and stale is not None:
        rows, asked_c, pos, ask_c = stale
        ov.stale_rows, ov.stale_pos = q(rows), q(pos)
        ov.stale_asked, ov.stale_ask = ctypes.cast(asked_c, ctypes.c_void_p), ctypes.cast(ask_c, ctypes.c_void_p)
    if next_plan_s is not None:
        ov.next_plan = ctypes.cast(ctypes.pointer(next_plan_s), ctypes.c_void_p)
        for i, b in enumerate(next_backs):
            ov.next_back[i] = b.data_ptr()
        for i, b in enumerate(next_serveds):
            ov.next_served[i] = q(b)
    ov.comm2 = getattr(comm2, "value", comm2)
    ov.side = side_stream.cuda_stream if side_stream is not None else None
    return ov


def overlap_release(ready):
    """Release a next_ready event that no call will consume (a loop that stopped early)."""
    if ready:
        _lib.load().esr_sharded_overlap_release(ready)


def sharded_triplet_step(group_s, plan_s, B, regularization, batch_size, lr, eps, device, overlap=None):
    """esr_sharded_triplet_step: lookup -> triplet loss on the rows where they landed -> update, one library call.
    Returns loss [1] (this rank's share).  overlap: a step_overlap_struct (esr_sharded_triplet_step_overlapped)."""
    lib = _lib.load()
    nb = int(lib.esr_sharded_triplet_step_workspace_bytes(ctypes.byref(group_s), ctypes.byref(plan_s), B))
    ov = ctypes.byref(overlap) if overlap is not None else None
    if ov is not None:
        nb += int(lib.esr_sharded_step_overlap_workspace_bytes(ctypes.byref(group_s), ov))
    ws = _ws(nb, device)
    loss = torch.empty(1, dtype=torch.float32, device=device)
    check(lib.esr_sharded_triplet_step_overlapped(ctypes.byref(group_s), ctypes.byref(plan_s), ov, B, float(regularization),
                                                  float(batch_size), float(lr), float(eps), _p(loss), _p(ws), ws.numel(),
                                                  _stream()), "esr_sharded_triplet_step")
    return loss


def sharded_glove_step(emb_s, bias_s, plan_s, target, B, mode, lr, eps, overlap=None):
    """esr_sharded_glove_step: both lookups -> GloVe loss -> both updates, one library call.  Returns loss [1].
    overlap: a step_overlap_struct (esr_sharded_glove_step_overlapped)."""
    lib = _lib.load()
    _req(target, torch.float32, "target")
    nb = int(lib.esr_sharded_glove_step_workspace_bytes(ctypes.byref(emb_s), ctypes.byref(bias_s), ctypes.byref(plan_s), B))
    ov = ctypes.byref(overlap) if overlap is not None else None
    if ov is not None:
        nb += int(lib.esr_sharded_step_overlap_workspace_bytes(ctypes.byref(emb_s), ov)) + \
            int(lib.esr_sharded_step_overlap_workspace_bytes(ctypes.byref(bias_s), ov))
    ws = _ws(nb, target.device)
    loss = torch.empty(1, dtype=torch.float32, device=target.device)
    check(lib.esr_sharded_glove_step_overlapped(ctypes.byref(emb_s), ctypes.byref(bias_s), ctypes.byref(plan_s), ov,
                                                _p(target), B, int(mode), float(lr), float(eps), _p(loss), _p(ws),
                                                ws.numel(), _stream()), "esr_sharded_glove_step")
    return loss


def rows_f32_to_bf16(rows):
    """[n, D] f32 -> bf16, round to nearest even (esr_rows_f32_to_bf16: what the bf16 gradient exchange sends)."""
    lib = _lib.load()
    _req(rows, torch.float32, "rows")
    out = torch.empty(rows.shape, dtype=torch.bfloat16, device=rows.device)
    check(lib.esr_rows_f32_to_bf16(_p(rows), rows.shape[0], rows.shape[1], _p(out), _stream()), "esr_rows_f32_to_bf16")
    return out


# ---------------------------------------------------------------------------------------------
# co-occurrence builder (esr_cooccur.hip): the table is one uint8 tensor, header words read through an int64 view
def cooccur_table(capacity, device):
    """A fresh, empty pair table of `capacity` (a power of two >= 2) slots."""
    lib = _lib.load()
    table = _ws(_ws_bytes("esr_cooccur_table_bytes", int(capacity)), device)
    check(lib.esr_cooccur_table_init(_p(table), int(capacity), _stream()), "esr_cooccur_table_init")
    return table


def cooccur_header(table):
    """(occupied slots, failure bits) of a pair table: one read-back, i.e. a sync."""
    used, fail = table[:16].view(torch.int64).tolist()
    return used, fail


def cooccur_accumulate(table, capacity, tokens, doc_offsets, tok_begin, tok_end, context_window):
    """Adds the window pairs whose later position lies in [tok_begin, tok_end) to the table."""
    lib = _lib.load()
    _req(tokens, torch.int32, "tokens"), _req(doc_offsets, torch.int64, "doc_offsets")
    check(lib.esr_cooccur_accumulate(_p(tokens), tokens.numel(), _p(doc_offsets), doc_offsets.numel() - 1,
                                     int(tok_begin), int(tok_end), int(context_window), _p(table), int(capacity),
                                     _stream()), "esr_cooccur_accumulate")


def cooccur_rehash(table, capacity, new_capacity):
    """A table of new_capacity slots holding every pair of `table` with its sum."""
    lib = _lib.load()
    new = _ws(_ws_bytes("esr_cooccur_table_bytes", int(new_capacity)), table.device)
    check(lib.esr_cooccur_rehash(_p(table), int(capacity), _p(new), int(new_capacity), _stream()), "esr_cooccur_rehash")
    return new


def cooccur_finalize(table, capacity, nnz, num_ids, context_window):
    """(index int32[nnz], other int32[nnz], count float32[nnz]) ascending by (index, other)."""
    lib = _lib.load()
    dev = table.device
    index = torch.empty(nnz, dtype=torch.int32, device=dev)
    other = torch.empty(nnz, dtype=torch.int32, device=dev)
    count = torch.empty(nnz, dtype=torch.float32, device=dev)
    ws = _ws(int(lib.esr_cooccur_finalize_workspace_bytes(int(nnz))), dev)
    check(lib.esr_cooccur_finalize(_p(table), int(capacity), int(nnz), int(num_ids), int(context_window), _p(index),
                                   _p(other), _p(count), _p(ws), ws.numel(), _stream()), "esr_cooccur_finalize")
    return index, other, count


# ---------------------------------------------------------------------------------------------
# set co-occurrence (Dice) builder (esr_dice.hip): it fills the pair table of the co-occurrence builder above
def dice_max_doc():
    """Ids a document may hold (esr_dice.hip sorts a document in LDS)."""
    return int(_lib.load().esr_dice_max_doc())


def dice_workspace(n_indices, device):
    """The workspace of dice_accumulate for an index array of n_indices ids."""
    return _ws(_ws_bytes("esr_dice_workspace_bytes", int(n_indices)), device)


def dice_accumulate(table, capacity, indices, doc_offsets, doc_begin, doc_end, workspace):
    """Adds the set pairs (and the document frequencies, on the diagonal keys) of documents [doc_begin, doc_end)."""
    lib = _lib.load()
    _req(indices, torch.int32, "indices"), _req(doc_offsets, torch.int64, "doc_offsets")
    check(lib.esr_dice_accumulate(_p(indices), indices.numel(), _p(doc_offsets), doc_offsets.numel() - 1,
                                  int(doc_begin), int(doc_end), _p(table), int(capacity), _p(workspace),
                                  workspace.numel(), _stream()), "esr_dice_accumulate")


# ---------------------------------------------------------------------------------------------
# term statistics, dictionary lookup, tf-idf rows (esr_terms.hip): pair tables of the co-occurrence builder above
def terms_accumulate(scratch, capacity, tokens, doc_offsets, doc_begin, doc_end, tok_begin, tok_end, lookup=None,
                     lookup_capacity=0):
    """tf of the whole documents [doc_begin, doc_end) = tokens [tok_begin, tok_end) into the scratch table, keyed
    (document - doc_begin) << 32 | id; id = the raw id, or its value in `lookup` (ids the lookup lacks are dropped)."""
    lib = _lib.load()
    _req(tokens, torch.int32, "tokens"), _req(doc_offsets, torch.int64, "doc_offsets")
    check(lib.esr_terms_accumulate(_p(tokens), tokens.numel(), _p(doc_offsets), doc_offsets.numel() - 1, int(doc_begin),
                                   int(doc_end), int(tok_begin), int(tok_end), _p(lookup), int(lookup_capacity),
                                   _p(scratch), int(capacity), _stream()), "esr_terms_accumulate")


def terms_fold(scratch, scratch_capacity, table, capacity):
    """Every (document, id, tf) of the scratch table: frequency[id] += tf, doc_frequency[id] += 1 in `table`."""
    check(_lib.load().esr_terms_fold(_p(scratch), int(scratch_capacity), _p(table), int(capacity), _stream()),
          "esr_terms_fold")


def terms_stats(table, capacity, n_ids):
    """(ids int32[n_ids], frequency int64[n_ids], doc_frequency int64[n_ids]) of a statistics table, in slot order."""
    dev = table.device
    ids = torch.empty(n_ids, dtype=torch.int32, device=dev)
    frequency = torch.empty(n_ids, dtype=torch.int64, device=dev)
    doc_frequency = torch.empty(n_ids, dtype=torch.int64, device=dev)
    counter = _ws(256, dev)
    check(_lib.load().esr_terms_stats(_p(table), int(capacity), int(n_ids), _p(ids), _p(frequency), _p(doc_frequency),
                                      _p(counter), _stream()), "esr_terms_stats")
    return ids, frequency, doc_frequency


def terms_lookup_table(keys, values, capacity):
    """A pair table of `capacity` >= 2 len(keys) slots with key = keys[i] (distinct raw ids), sum = values[i]."""
    _req(keys, torch.int32, "keys"), _req(values, torch.int32, "values")
    table = cooccur_table(capacity, keys.device)
    check(_lib.load().esr_terms_lookup_build(_p(keys), _p(values), keys.numel(), _p(table), int(capacity), _stream()),
          "esr_terms_lookup_build")
    return table


def terms_lookup(tokens, lookup, lookup_capacity, mode, size, oov_bucket=None):
    """(out int32[N], fail int64[1]): mode 0 the value of each token or -1; mode 1 the embedding index (1 + value, or
    1 + size + bucket).  fail holds bit 2 (a negative token) / bit 32 (a bucket outside [0, 65536)); reading it syncs."""
    _req(tokens, torch.int32, "tokens")
    if oov_bucket is not None:
        _req(oov_bucket, torch.int32, "oov_bucket")
    out = torch.empty(tokens.numel(), dtype=torch.int32, device=tokens.device)
    fail = torch.zeros(1, dtype=torch.int64, device=tokens.device)
    check(_lib.load().esr_terms_lookup(_p(tokens), tokens.numel(), _p(lookup), int(lookup_capacity), int(mode), int(size),
                                       _p(oov_bucket), _p(out), _p(fail), _stream()), "esr_terms_lookup")
    return out, fail


def terms_tfidf_rows(scratch, capacity, index, row_off, idf):
    """float32[nnz]: the L2-normalised tf * idf of the rows row_off (int32 [nrows + 1]) of `index`, tf read from scratch."""
    _req(index, torch.int32, "index"), _req(row_off, torch.int32, "row_off"), _req(idf, torch.float64, "idf")
    out = torch.empty(index.numel(), dtype=torch.float32, device=index.device)
    check(_lib.load().esr_terms_tfidf_rows(_p(scratch), int(capacity), _p(index), _p(row_off), row_off.numel() - 1,
                                           index.numel(), _p(idf), idf.numel(), _p(out), _stream()),
          "esr_terms_tfidf_rows")
    return out


# ---------------------------------------------------------------------------------------------
# item-to-item neighbours and the item-kNN recommender (esr_neighbours.hip)
def neighbours_plan_bounds():
    """The row lengths at which the neighbour select changes class, ascending (esr_neighbours_plan_bounds)."""
    lib = _lib.load()
    n = int(lib.esr_neighbours_plan_bounds(None, 0))
    buf = (ctypes.c_int32 * n)()
    lib.esr_neighbours_plan_bounds(ctypes.addressof(buf), n)
    return list(buf)


def neighbours_topk(index, other, count, ids, df, k, both, dice):
    """(neighbours int32[u, k], scores float32[u, k], counts float32[u, k], lengths int32[u], fail int) of the rows of
    `ids`; fail = the failure word of the call (bit 64: an entry with an id that `ids` lacks).  Reading it syncs."""
    lib = _lib.load()
    _req(index, torch.int32, "index"), _req(other, torch.int32, "other"), _req(count, torch.float32, "count")
    _req(ids, torch.int32, "ids")
    if df is not None:
        _req(df, torch.float32, "df")
    dev, nnz, u = ids.device, index.numel(), ids.numel()
    nb = torch.empty((u, k), dtype=torch.int32, device=dev)
    scores = torch.empty((u, k), dtype=torch.float32, device=dev)
    counts = torch.empty((u, k), dtype=torch.float32, device=dev)
    lengths = torch.empty(u, dtype=torch.int32, device=dev)
    ws = _ws(int(lib.esr_neighbours_workspace_bytes(nnz, u, int(both))), dev)
    check(lib.esr_neighbours_topk(_p(index), _p(other), _p(count), nnz, _p(ids), _p(df), u, int(k), int(both), int(dice),
                                  _p(nb), _p(scores), _p(counts), _p(lengths), _p(ws), ws.numel(), _stream()),
          "esr_neighbours_topk")
    fail = int(ws[:8].view(torch.int64).item()) if u and nnz else 0
    return nb, scores, counts, lengths, fail


def itemknn_max_entries():
    """History length x table width one query of itemknn_recommend may gather (one workgroup sorts them in LDS)."""
    return int(_lib.load().esr_itemknn_max_entries())


def itemknn_recommend(table_ids, table_neighbours, table_scores, table_lengths, history, offsets, k, exclude_history):
    """(ids int32[nq, k], scores float32[nq, k], lengths int32[nq]) of the queries history[offsets[q]:offsets[q + 1]]."""
    lib = _lib.load()
    _req(table_ids, torch.int32, "table.ids"), _req(table_neighbours, torch.int32, "table.neighbours")
    _req(table_scores, torch.float32, "table.scores"), _req(table_lengths, torch.int32, "table.lengths")
    _req(history, torch.int32, "history"), _req(offsets, torch.int64, "offsets")
    dev, nq = history.device, offsets.numel() - 1
    out_ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_lengths = torch.empty(nq, dtype=torch.int32, device=dev)
    check(lib.esr_itemknn_recommend(_p(table_ids), _p(table_neighbours), _p(table_scores), _p(table_lengths),
                                    table_ids.numel(), int(table_neighbours.shape[1]), _p(history), history.numel(),
                                    _p(offsets), nq, int(k), int(bool(exclude_history)), _p(out_ids), _p(out_scores),
                                    _p(out_lengths), _stream()), "esr_itemknn_recommend")
    return out_ids, out_scores, out_lengths


# ---------------------------------------------------------------------------------------------
# ranking metrics of recommended lists against held-out truth sets (esr_eval.hip)
def eval_max_truth():
    """Distinct truth ids one query of eval_ranking may hold (its table in LDS)."""
    return int(_lib.load().esr_eval_max_truth())


def eval_max_width():
    """The widest list eval_ranking scores."""
    return int(_lib.load().esr_eval_max_width())


def eval_ranking(rec_ids, rec_lengths, truth, truth_offsets, max_truth, ks, disc, cum_disc, count_repeats, listed):
    """esr_eval_ranking: a dict of device tensors -- hits int32[nq, nk], first_hit / valid int32[nq], precision, recall,
    rr, ap, ndcg float32[nq, nk] (ap and ndcg None with count_repeats) -- and the failure word (reading it syncs).
    rec_ids int32[nq, width] with unit stride along a row (any row pitch); ks a sequence of ints (host); disc /
    cum_disc float64 device tensors as include/esr_hip.h describes them."""
    lib = _lib.load()
    if not isinstance(rec_ids, torch.Tensor) or not rec_ids.is_cuda:
        raise TypeError("rec_ids must be a CUDA/ROCm tensor (no CPU fallback exists)")
    if rec_ids.dtype != torch.int32 or rec_ids.dim() != 2 or (rec_ids.shape[1] > 1 and rec_ids.stride(1) != 1):
        raise TypeError("rec_ids must be int32 [nq, width] with unit stride along a row")
    if rec_lengths is not None:
        _req(rec_lengths, torch.int32, "rec_lengths")
    _req(truth, torch.int32, "truth"), _req(truth_offsets, torch.int64, "truth_offsets")
    _req(disc, torch.float64, "disc"), _req(cum_disc, torch.float64, "cum_disc")
    dev, (nq, width) = rec_ids.device, rec_ids.shape
    pitch = rec_ids.stride(0) if nq > 1 else width
    nk = len(ks)
    ks_host = (ctypes.c_int32 * max(nk, 1))(*[int(k) for k in ks])
    out = {"hits": torch.empty((nq, nk), dtype=torch.int32, device=dev),
           "first_hit": torch.empty(nq, dtype=torch.int32, device=dev),
           "valid": torch.empty(nq, dtype=torch.int32, device=dev)}
    for name in ("precision", "recall", "rr") + (() if count_repeats else ("ap", "ndcg")):
        out[name] = torch.empty((nq, nk), dtype=torch.float32, device=dev)
    out.setdefault("ap", None), out.setdefault("ndcg", None)
    fail = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib.esr_eval_ranking(_p(rec_ids), int(pitch), int(width), _p(rec_lengths), _p(truth), truth.numel(),
                               _p(truth_offsets), nq, int(max_truth), ctypes.addressof(ks_host), nk, _p(disc), _p(cum_disc),
                               int(bool(count_repeats)), int(bool(listed)), _p(out["hits"]), _p(out["first_hit"]),
                               _p(out["valid"]), _p(out["precision"]), _p(out["recall"]), _p(out["rr"]), _p(out["ap"]),
                               _p(out["ndcg"]), _p(fail), _stream()), "esr_eval_ranking")
    return out, (int(fail.item()) if nq else 0)


# ---------------------------------------------------------------------------------------------
# explicit ratings: the wide pair table, Pearson user similarity and the user-kNN affinity (esr_ratings.hip)
def usersim_tile():
    """T: the raters per chunk of the accumulate kernel; an item of n >= 2 raters is ceil(n / T) chunks."""
    return int(_lib.load().esr_usersim_tile())


def usersim_table(capacity, device):
    """A fresh, empty WIDE pair table (four sums per slot) of `capacity` (a power of two >= 2) slots."""
    lib = _lib.load()
    table = _ws(_ws_bytes("esr_usersim_table_bytes", int(capacity)), device)
    check(lib.esr_usersim_table_init(_p(table), int(capacity), _stream()), "esr_usersim_table_init")
    return table


def usersim_rehash(table, capacity, new_capacity):
    """A wide table of new_capacity slots holding every pair of `table` with its four sums."""
    lib = _lib.load()
    new = _ws(_ws_bytes("esr_usersim_table_bytes", int(new_capacity)), table.device)
    check(lib.esr_usersim_rehash(_p(table), int(capacity), _p(new), int(new_capacity), _stream()), "esr_usersim_rehash")
    return new


def usersim_accumulate(table, capacity, users, dev, item_offsets, item_ids, tile_prefix, item_begin, item_end, ntiles):
    """Adds the user pairs of the items [item_begin, item_end) of the CSR-by-item ratings (users ascending inside an item)."""
    lib = _lib.load()
    _req(users, torch.int32, "users"), _req(dev, torch.int32, "dev"), _req(item_offsets, torch.int64, "item_offsets")
    _req(item_ids, torch.int32, "item_ids"), _req(tile_prefix, torch.int64, "tile_prefix")
    check(lib.esr_usersim_accumulate(_p(users), _p(dev), users.numel(), _p(item_offsets), _p(item_ids), _p(tile_prefix),
                                     item_offsets.numel() - 1, int(item_begin), int(item_end), int(ntiles), _p(table),
                                     int(capacity), _stream()), "esr_usersim_accumulate")


def usersim_finalize(table, capacity, nnz, num_ids, min_overlap, min_similarity):
    """(index int32[kept], other int32[kept], sim float32[kept], overlap int32[kept], dropped_flat): the kept rows
    ascending by (index, other).  Reading the two counts syncs."""
    lib = _lib.load()
    dev = table.device
    index = torch.empty(nnz, dtype=torch.int32, device=dev)
    other = torch.empty(nnz, dtype=torch.int32, device=dev)
    sim = torch.empty(nnz, dtype=torch.float32, device=dev)
    overlap = torch.empty(nnz, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = _ws(int(lib.esr_usersim_finalize_workspace_bytes(int(nnz))), dev)
    check(lib.esr_usersim_finalize(_p(table), int(capacity), int(nnz), int(num_ids), int(min_overlap),
                                   int(min_similarity is not None), float(min_similarity or 0.0), _p(index), _p(other),
                                   _p(sim), _p(overlap), _p(counts), _p(ws), ws.numel(), _stream()), "esr_usersim_finalize")
    kept, flat = counts.tolist()
    return index[:kept], other[:kept], sim[:kept], overlap[:kept], flat


def userknn_max_entries():
    """The ratings of all neighbours that one query of userknn_recommend may gather (one workgroup sorts them in LDS)."""
    return int(_lib.load().esr_userknn_max_entries())


def _userknn_args(table_ids, table_neighbours, table_scores, table_lengths, users, row_offsets, items, ratings, mean):
    _req(table_ids, torch.int32, "table.ids"), _req(table_neighbours, torch.int32, "table.neighbours")
    _req(table_scores, torch.float32, "table.scores"), _req(table_lengths, torch.int32, "table.lengths")
    _req(users, torch.int32, "users"), _req(row_offsets, torch.int64, "row_offsets"), _req(items, torch.int32, "items")
    _req(ratings, torch.float32, "ratings"), _req(mean, torch.float64, "mean")
    return (_p(table_ids), _p(table_neighbours), _p(table_scores), _p(table_lengths), table_ids.numel(),
            int(table_neighbours.shape[1]), _p(users), users.numel(), _p(row_offsets), _p(items), _p(ratings), items.numel(),
            _p(mean))


def userknn_predict(table_ids, table_neighbours, table_scores, table_lengths, users, row_offsets, items, ratings, mean,
                    query_users, query_items, center_neighbour, den_all):
    """(affinity float32[nq], support int32[nq]) of the (user, item) queries."""
    lib = _lib.load()
    args = _userknn_args(table_ids, table_neighbours, table_scores, table_lengths, users, row_offsets, items, ratings, mean)
    _req(query_users, torch.int32, "query_users"), _req(query_items, torch.int32, "query_items")
    nq = query_users.numel()
    aff = torch.empty(nq, dtype=torch.float32, device=users.device)
    support = torch.empty(nq, dtype=torch.int32, device=users.device)
    check(lib.esr_userknn_predict(*args, _p(query_users), _p(query_items), nq, int(bool(center_neighbour)),
                                  int(bool(den_all)), _p(aff), _p(support), _stream()), "esr_userknn_predict")
    return aff, support


def userknn_recommend(table_ids, table_neighbours, table_scores, table_lengths, users, row_offsets, items, ratings, mean,
                      query_users, k, exclude_rated, min_support, center_neighbour, den_all):
    """(ids int32[nq, k], scores float32[nq, k], lengths int32[nq]) of the query users."""
    lib = _lib.load()
    args = _userknn_args(table_ids, table_neighbours, table_scores, table_lengths, users, row_offsets, items, ratings, mean)
    _req(query_users, torch.int32, "query_users")
    dev, nq = users.device, query_users.numel()
    out_ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_lengths = torch.empty(nq, dtype=torch.int32, device=dev)
    check(lib.esr_userknn_recommend(*args, _p(query_users), nq, int(k), int(bool(exclude_rated)), int(min_support),
                                    int(bool(center_neighbour)), int(bool(den_all)), _p(out_ids), _p(out_scores),
                                    _p(out_lengths), _stream()), "esr_userknn_recommend")
    return out_ids, out_scores, out_lengths


# ---------------------------------------------------------------------------------------------
# matrix factorisation of explicit ratings by alternating least squares (esr_als.hip)
def als_max_rank():
    """The largest rank esr_als_solve_rows and esr_als_gram take."""
    return int(_lib.load().esr_als_max_rank())


def als_predict_max_rank():
    """The widest row esr_als_predict takes: a per-pair loop, so the row-group cap of bpr_geometry() and not als_max_rank()."""
    return int(_lib.load().esr_als_predict_max_rank())


def als_geometry():
    """(chunk, chunks_per_workgroup): a row's ratings are cut into chunks of `chunk` consecutive ratings; a wave solves a
    row of up to one chunk, a workgroup one of up to chunks_per_workgroup chunks, longer rows go through workspace partials."""
    chunk, per_wg = ctypes.c_int(0), ctypes.c_int(0)
    check(_lib.load().esr_als_geometry(ctypes.byref(chunk), ctypes.byref(per_wg)), "esr_als_geometry")
    return int(chunk.value), int(per_wg.value)


def _als_solve(name, other_factors, row_offsets, cols, values, what, row_begin, row_end, reg, weighted, out_factors,
               failed, gram=None):
    """What als_solve_rows and als_solve_rows_implicit share: the checks, the workspace and the one library call
    (`gram` goes in after the rank when given)."""
    lib = _lib.load()
    _req(other_factors, torch.float32, "other_factors"), _req(out_factors, torch.float32, "out_factors")
    if gram is not None:
        _req(gram, torch.float32, "gram")
    _req(cols, torch.int32, "cols"), _req(values, torch.float32, what), _req(failed, torch.int32, "failed")
    if not isinstance(row_offsets, np.ndarray) or row_offsets.dtype != np.int64 or not row_offsets.flags.c_contiguous:
        raise TypeError("row_offsets must be a contiguous numpy int64 array (host memory)")
    row_begin, row_end = int(row_begin), int(row_end)
    if not 0 <= row_begin <= row_end < row_offsets.size:
        raise ValueError("rows [%d, %d) not inside the %d rows of row_offsets" % (row_begin, row_end, row_offsets.size - 1))
    if out_factors.shape[0] < row_end or out_factors.shape[1] != other_factors.shape[1]:
        raise ValueError("out_factors %s does not hold rows up to %d of rank %d"
                         % (tuple(out_factors.shape), row_end, other_factors.shape[1]))
    n_other, rank = other_factors.shape
    if gram is not None and tuple(gram.shape) != (rank, rank):
        raise ValueError("gram %s is not [%d, %d]" % (tuple(gram.shape), rank, rank))
    if int(row_offsets[row_end]) > cols.numel() or cols.numel() != values.numel():
        raise ValueError("row_offsets end at %d but there are %d cols and %d %s"
                         % (int(row_offsets[row_end]), cols.numel(), values.numel(), what))
    nnz = int(row_offsets[row_end] - row_offsets[row_begin])
    ws = _ws(int(lib.esr_als_solve_workspace_bytes(row_end - row_begin, nnz, int(rank))), out_factors.device)
    check(getattr(lib, name)(_p(other_factors), int(n_other), int(rank), *(() if gram is None else (_p(gram),)), row_offsets.ctypes.data,
                      _p(cols), _p(values), row_begin, row_end, float(reg), int(bool(weighted)), _p(out_factors), _p(failed),
                      _p(ws), ws.numel(), _stream()), name)


def als_solve_rows(other_factors, row_offsets, cols, targets, row_begin, row_end, reg, weighted, out_factors, failed):
    """One half-sweep over the rows [row_begin, row_end): out_factors[r] = the regularised least-squares solution of row r's
    ratings against other_factors.  row_offsets is a HOST array (numpy int64[n_rows + 1]): the library sorts the rows into
    its three classes from it.  `failed` (int32[1], device) collects the failure word; the caller zeroes and reads it."""
    _als_solve("esr_als_solve_rows", other_factors, row_offsets, cols, targets, "targets", row_begin, row_end, reg, weighted,
               out_factors, failed)


def als_predict(user_factors, item_factors, user_pos, item_pos, offset=None, targets=None):
    """float32[nq]: float32(offset[u] + x_u . y_i) with the dot product summed in fp64 in ascending dimension (NaN where a
    position is outside its table); with `targets` the residual float32(float64(targets) - that)."""
    lib = _lib.load()
    _req(user_factors, torch.float32, "user_factors"), _req(item_factors, torch.float32, "item_factors")
    _req(user_pos, torch.int32, "user_pos"), _req(item_pos, torch.int32, "item_pos")
    if offset is not None:
        _req(offset, torch.float64, "offset")
        if offset.numel() != user_factors.shape[0]:
            raise ValueError("offset must have one entry per user row")
    if targets is not None:
        _req(targets, torch.float32, "targets")
    nq = user_pos.numel()
    if item_pos.numel() != nq or (targets is not None and targets.numel() != nq):
        raise ValueError("user_pos, item_pos (and targets) must have one length")
    if user_factors.shape[1] != item_factors.shape[1]:
        raise ValueError("user_factors and item_factors differ in rank")
    out = torch.empty(nq, dtype=torch.float32, device=user_factors.device)
    check(lib.esr_als_predict(_p(user_factors), user_factors.shape[0], _p(item_factors), item_factors.shape[0],
                              int(user_factors.shape[1]), _p(user_pos), _p(item_pos), _p(offset), _p(targets), nq, _p(out),
                              _stream()), "esr_als_predict")
    return out


# implicit-feedback ALS: the whole-table Gram matrix and the confidence-weighted row solve (esr_als.hip)
def als_gram_geometry():
    """segment: esr_als_gram cuts the table into segments of that many consecutive rows, one f32 chain per entry each."""
    segment = ctypes.c_int(0)
    check(_lib.load().esr_als_gram_geometry(ctypes.byref(segment)), "esr_als_gram_geometry")
    return int(segment.value)


def als_gram(factors, out=None):
    """float32[rank, rank] = factors^T factors of a float32 table [n, rank] (the full symmetric matrix): per segment of
    als_gram_geometry() rows a k-ordered f32 chain, the segments added in fp64 in ascending order and rounded once."""
    lib = _lib.load()
    _req(factors, torch.float32, "factors")
    if factors.dim() != 2:
        raise ValueError("factors must be [n, rank]")
    n, rank = factors.shape
    if out is None:
        out = torch.empty((rank, rank), dtype=torch.float32, device=factors.device)
    _req(out, torch.float32, "out")
    if tuple(out.shape) != (rank, rank):
        raise ValueError("out %s is not [%d, %d]" % (tuple(out.shape), rank, rank))
    ws = _ws(int(lib.esr_als_gram_workspace_bytes(int(n), int(rank))), factors.device)
    check(lib.esr_als_gram(_p(factors), int(n), int(rank), _p(out), _p(ws), ws.numel(), _stream()), "esr_als_gram")
    return out


def als_solve_rows_implicit(other_factors, gram, row_offsets, cols, weights, row_begin, row_end, reg, weighted, out_factors,
                            failed):
    """One implicit-feedback half-sweep over the rows [row_begin, row_end): out_factors[r] solves
    (gram + sum_k w_k y_k y_k^T + lam I) x = sum_k (1 + w_k) y_k over row r's entries.  `gram` is als_gram(other_factors);
    row_offsets is a HOST array (numpy int64[n_rows + 1]) as in als_solve_rows; `failed` (int32[1], device) collects the
    failure word (bit 30: a column outside the table, bit 29: a weight that is negative or not finite)."""
    _als_solve("esr_als_solve_rows_implicit", other_factors, row_offsets, cols, weights, "weights", row_begin, row_end, reg,
               weighted, out_factors, failed, gram=gram)


# ---------------------------------------------------------------------------------------------
# Bayesian Personalised Ranking (esr_bpr.hip): the triple sampler and the fused logistic forward / backward
def _failed_word(failed, device):
    """`failed`, or a fresh scratch word on `device` when None."""
    if failed is None:
        failed = torch.zeros(1, dtype=torch.int32, device=device)
    _req(failed, torch.int32, "failed")
    return failed


def _check_rank4(D, top, mult):
    if D % mult or not mult <= D <= top:
        raise ValueError("rank = %d is not a multiple of %d in [%d, %d]" % (D, mult, mult, top))


def _check_device_csr(who, name, offsets, row_upos, row_ipos, nu, **sizes):
    """The CSR of seen pairs by user on the device, as bpr_sample and warp_step take it; every one of nu, nnz and `sizes` in
    [1, 2^31 - 1].  Returns nnz."""
    _req(offsets, torch.int64, name), _req(row_upos, torch.int32, "row_upos"), _req(row_ipos, torch.int32, "row_ipos")
    nnz = row_upos.numel()
    if row_ipos.numel() != nnz or offsets.numel() != nu + 1:
        raise ValueError("%s: %s holds %d entries for nu = %d, row_upos %d and row_ipos %d pairs"
                         % (who, name, offsets.numel(), nu, nnz, row_ipos.numel()))
    sizes = dict(nu=nu, nnz=nnz, **sizes)
    if not all(1 <= v <= 2 ** 31 - 1 for v in sizes.values()):
        raise ValueError("%s: %s (each in [1, 2^31 - 1])" % (who, " ".join("%s=%d" % kv for kv in sizes.items())))
    return nnz


def _geometry(name, n):
    """The n ints esr_<name>_geometry() fills, as a tuple."""
    out = [ctypes.c_int(0) for _ in range(n)]
    check(getattr(_lib.load(), "esr_%s_geometry" % name)(*[ctypes.byref(v) for v in out]), "esr_%s_geometry" % name)
    return tuple(int(v.value) for v in out)


def _check_valid(valid, n, per, who=""):
    """valid is None (all valid) or int32[n]."""
    if valid is not None:
        _req(valid, torch.int32, "valid")
        if valid.numel() != n:
            raise ValueError("%svalid must hold one entry per %s" % (who, per))


def _sample_outputs(n, K, B, dev):
    """(the n id planes int32[n, K, B] of a sampler, dropped int32[K])"""
    return torch.empty((n, K, B), dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int32, device=dev)


def _step_outputs(B, rows, D, dev, want_grads, want_diff, scores=None):
    """(loss_t float32[B], diff_t float32[B] -- [B, scores] with `scores` -- or None, grads float32[rows, D] or None)"""
    loss_t = torch.empty(B, dtype=torch.float32, device=dev)
    diff_t = torch.empty(B if scores is None else (B, scores), dtype=torch.float32, device=dev) if want_diff else None
    return loss_t, diff_t, torch.empty((rows, D), dtype=torch.float32, device=dev) if want_grads else None


def bpr_geometry():
    """(max_tries, max_rank, rank_multiple): the negative candidates the sampler tries per triple; bpr_fwd_bwd takes a rank
    that is a multiple of rank_multiple and at most max_rank."""
    return _geometry("bpr", 3)


def bpr_sample(row_offsets, row_upos, row_ipos, nu, ni, seed, step0, K, B):
    """K steps of B (user, seen item, unseen item) triples drawn on the device: (u, i, j, valid) int32 [K, B] -- row k is
    global step step0 + k (mod 2^32) -- and dropped int32[K], the count of valid == 0 per step.  The seen pairs are a CSR by
    user on the DEVICE: row_offsets int64[nu + 1], row_upos / row_ipos int32[nnz], item positions ascending within a row.
    The rule is esr_bpr_sample.h's: a triple is a function of (seed, step, slot, CSR) alone; the multiply-high draws are
    biased by at most nnz / 2^32 (the pair) and ni / 2^32 (a candidate) relative."""
    lib = _lib.load()
    nu, ni, K, B = int(nu), int(ni), int(K), int(B)
    nnz = _check_device_csr("bpr_sample", "row_offsets", row_offsets, row_upos, row_ipos, nu, ni=ni, K=K, B=B)
    out, dropped = _sample_outputs(4, K, B, row_upos.device)
    check(lib.esr_bpr_sample(_p(row_offsets), _p(row_upos), _p(row_ipos), nu, ni, nnz, int(seed) & (2 ** 64 - 1),
                             int(step0) & 0xFFFFFFFF, K, B, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _p(dropped),
                             _stream()), "esr_bpr_sample")
    return out[0], out[1], out[2], out[3], dropped


def bpr_fwd_bwd(user_table, item_table, u, i, j, valid, reg, want_grads=True, want_diff=False, failed=None):
    """(loss_t float32[B], diff_t float32[B] or None, grads float32[3 B, D] or None) of the triples (u, i, j) int32[B]:
    d = x_u . (y_i - y_j), loss_t = softplus(-d), diff_t = d, and the gradient rows [user ; positive ; negative] in
    occurrence order with the L2 term reg * row (include/esr_hip.h).  valid int32[B] or None (all valid): a triple with
    valid = 0 gives zeros.  `failed` (int32[1], device; a scratch word when None) gets bit 30 when an id lies outside its
    table -- that triple gives zeros too; the caller zeroes and reads it."""
    lib = _lib.load()
    _req(user_table, torch.float32, "user_table"), _req(item_table, torch.float32, "item_table")
    _req(u, torch.int32, "u"), _req(i, torch.int32, "i"), _req(j, torch.int32, "j")
    if user_table.dim() != 2 or item_table.dim() != 2 or user_table.shape[1] != item_table.shape[1]:
        raise ValueError("user_table and item_table must be [n, rank] of one rank")
    B, D = u.numel(), int(user_table.shape[1])
    if i.numel() != B or j.numel() != B:
        raise ValueError("u, i and j must have one length")
    _check_valid(valid, B, "triple")
    _check_rank4(D, *bpr_geometry()[1:])
    dev = user_table.device
    failed = _failed_word(failed, dev)
    loss_t, diff_t, grads = _step_outputs(B, 3 * B, D, dev, want_grads, want_diff)
    if B:
        check(lib.esr_bpr_fwd_bwd(_p(user_table), user_table.shape[0], _p(item_table), item_table.shape[0], D, _p(u), _p(i),
                                  _p(j), _p(valid), B, float(reg), _p(loss_t), _p(diff_t), _p(grads), _p(failed), _stream()),
              "esr_bpr_fwd_bwd")
    return loss_t, diff_t, grads


# ---------------------------------------------------------------------------------------------
# WARP (esr_warp.hip): the fused sample / score / search / weight / gradient step
def warp_geometry():
    """(max_trials, max_rank, rank_multiple): the most candidates one search may walk; warp_step takes a rank that is a
    multiple of rank_multiple and at most max_rank."""
    return _geometry("warp", 3)


def warp_step(user_factors, item_factors, offsets, row_upos, row_ipos, rank_weight, seed, step, B, max_trials, margin, reg,
              want_grads=True, want_diff=False, failed=None):
    """One WARP step of B slots in one launch: (u, i, j, valid, trials) int32[B], loss_t float32[B], diff float32[B] or None
    and grads float32[3 B, D] or None.  The seen pairs are bpr_sample's CSR on the DEVICE (offsets int64[nu + 1], row_upos /
    row_ipos int32[nnz]); rank_weight is float32[ni + 1].  The rule is esr_warp_sample.h's: the pair and the candidates
    come from bpr_sample's Philox stream; the first unseen candidate within max_trials whose d = x_u . y_i - x_u . y_j is
    below margin is the negative, trials counts the unseen candidates walked, w = rank_weight[max(1, (ni - len_u) //
    trials)], loss_t = w (margin - d) and grads = [user ; positive ; negative] rows with the L2 term reg * row.  A slot
    without a violating candidate has valid = 0 and zeros.  `failed` (int32[1], device; a scratch word when None) gets
    bit 30 when an item position lies outside the table; the caller zeroes and reads it."""
    lib = _lib.load()
    _req(user_factors, torch.float32, "user_factors"), _req(item_factors, torch.float32, "item_factors")
    _req(rank_weight, torch.float32, "rank_weight")
    if user_factors.dim() != 2 or item_factors.dim() != 2 or user_factors.shape[1] != item_factors.shape[1]:
        raise ValueError("user_factors and item_factors must be [n, rank] of one rank")
    nu, ni, D, B = int(user_factors.shape[0]), int(item_factors.shape[0]), int(user_factors.shape[1]), int(B)
    if rank_weight.numel() != ni + 1:
        raise ValueError("warp_step: rank_weight holds %d entries for ni = %d" % (rank_weight.numel(), ni))
    nnz = _check_device_csr("warp_step", "offsets", offsets, row_upos, row_ipos, nu, ni=ni, B=B)
    top_trials, max_rank, mult = warp_geometry()
    _check_rank4(D, max_rank, mult)
    max_trials = int(max_trials)
    if not 1 <= max_trials <= top_trials:
        raise ValueError("max_trials = %d outside [1, %d]" % (max_trials, top_trials))
    dev = user_factors.device
    failed = _failed_word(failed, dev)
    ids = torch.empty((5, B), dtype=torch.int32, device=dev)
    loss_t, diff, grads = _step_outputs(B, 3 * B, D, dev, want_grads, want_diff)
    check(lib.esr_warp_step(_p(user_factors), nu, _p(item_factors), ni, D, _p(offsets), _p(row_upos), _p(row_ipos), nnz,
                            _p(rank_weight), int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, B, max_trials, float(margin),
                            float(reg), _p(ids[0]), _p(ids[1]), _p(ids[2]), _p(ids[3]), _p(ids[4]), _p(loss_t), _p(diff),
                            _p(grads), _p(failed), _stream()), "esr_warp_step")
    return ids[0], ids[1], ids[2], ids[3], ids[4], loss_t, diff, grads


# ---------------------------------------------------------------------------------------------
# Bag tables (esr_bag.hip): rows composed as weighted sums of feature rows, and the transpose for the optimiser
def bag_geometry():
    """(max_rank, rank_multiple): bag_sum and bag_expand take a rank that is a multiple of rank_multiple and at most
    max_rank -- bpr_fwd_bwd's geometry."""
    return _geometry("bag", 2)


def _bag_args(who, table, offsets, feat, weight, rows):
    """The checks bag_sum and bag_expand share.  Returns (nf, D, nnz, n_bags, n)."""
    _req(table, torch.float32, "table"), _req(offsets, torch.int64, "offsets"), _req(feat, torch.int32, "feat")
    if table.dim() != 2:
        raise ValueError("%s: table must be [nf, rank]" % who)
    nf, D, nnz, n_bags = int(table.shape[0]), int(table.shape[1]), feat.numel(), offsets.numel() - 1
    _check_rank4(D, *bag_geometry())
    if weight is not None:
        _req(weight, torch.float32, "weight")
        if weight.numel() != nnz:
            raise ValueError("%s: weight must hold one entry per feat entry" % who)
    lim = 2 ** 31 - 1
    if not (1 <= nf <= lim and 1 <= nnz <= lim and 1 <= n_bags <= lim):
        raise ValueError("%s: nf=%d nnz=%d n_bags=%d (each in [1, 2^31 - 1])" % (who, nf, nnz, n_bags))
    if rows is not None:
        _req(rows, torch.int32, "rows")
    n = n_bags if rows is None else rows.numel()
    if n > lim:
        raise ValueError("%s: n=%d above 2^31 - 1" % (who, n))
    return nf, D, nnz, n_bags, n


def bag_sum(table, offsets, feat, weight, rows=None, out=None, failed=None):
    """out float32[n, D]: row r is the bag b = rows[r] (int32[n], any order, repeats allowed; every bag in order when None)
    of the bag table (offsets int64[n_bags + 1], feat int32[nnz] positions into table float32[nf, D], weight float32[nnz]
    or None = all 1) composed by the rule of esr_bag_rule.h: acc = fmaf(w[k], table[feat[k]], acc) over the bag's
    occurrences in ascending order from +0.0.  An empty bag gives zeros.  `failed` (int32[1], device; a scratch word when
    None) gets bit 30 when a bag number or feature position lies outside its table -- that row is zeros; the caller zeroes
    and reads it."""
    lib = _lib.load()
    nf, D, nnz, n_bags, n = _bag_args("bag_sum", table, offsets, feat, weight, rows)
    dev = table.device
    if out is None:
        out = torch.empty((n, D), dtype=torch.float32, device=dev)
    _req(out, torch.float32, "out")
    if out.numel() != n * D:
        raise ValueError("bag_sum: out must be [n, rank]")
    failed = _failed_word(failed, dev)
    if n:
        check(lib.esr_bag_sum(_p(table), nf, D, _p(offsets), _p(feat), _p(weight), nnz, n_bags, _p(rows), n, _p(out),
                              _p(failed), _stream()), "esr_bag_sum")
    return out


def bag_expand(table, offsets, feat, weight, rows, grad_rows, valid, out_offsets, M, reg, out=None, failed=None):
    """(out_feat int32[M], out_grads float32[M, D]): the gradients grad_rows float32[n, D] of the rows bag_sum composed for
    `rows`, handed to the features as one row per occurrence: occurrence k of selected bag r lands at p = out_offsets[r] +
    (k - offsets[b]) with out_feat[p] = feat[k] and out_grads[p] = fmaf(w[k], grad_rows[r], reg * table[feat[k]]).
    out_offsets int64[n + 1] is the exclusive scan of the selected bags' lengths and M = out_offsets[n], both computed by
    the caller.  valid int32[n] or None (all valid): valid[r] == 0 gives zero rows and the table is not read.  `out` = an
    (out_feat, out_grads) pair to write into.  `failed` as bag_sum's; a refused occurrence gives out_feat = 0 and zeros."""
    lib = _lib.load()
    nf, D, nnz, n_bags, n = _bag_args("bag_expand", table, offsets, feat, weight, rows)
    _req(grad_rows, torch.float32, "grad_rows"), _req(out_offsets, torch.int64, "out_offsets")
    M = int(M)
    if grad_rows.numel() != n * D or out_offsets.numel() != n + 1:
        raise ValueError("bag_expand: grad_rows must be [n, rank] and out_offsets hold n + 1 entries")
    if not 0 <= M <= 2 ** 31 - 1:
        raise ValueError("bag_expand: M=%d expanded occurrences outside [0, 2^31 - 1]" % M)
    _check_valid(valid, n, "selected bag", "bag_expand: ")
    dev = table.device
    if out is None:
        out = (torch.empty(M, dtype=torch.int32, device=dev), torch.empty((M, D), dtype=torch.float32, device=dev))
    out_feat, out_grads = out
    _req(out_feat, torch.int32, "out[0]"), _req(out_grads, torch.float32, "out[1]")
    if out_feat.numel() != M or out_grads.numel() != M * D:
        raise ValueError("bag_expand: out must be (int32[M], float32[M, rank])")
    failed = _failed_word(failed, dev)
    if n:
        check(lib.esr_bag_expand(_p(table), nf, D, _p(offsets), _p(feat), _p(weight), nnz, n_bags, _p(rows), _p(grad_rows),
                                 _p(valid), _p(out_offsets), n, M, float(reg), _p(out_feat), _p(out_grads), _p(failed),
                                 _stream()), "esr_bag_expand")
    return out_feat, out_grads


# ---------------------------------------------------------------------------------------------
# Factorised Personalised Markov Chain (esr_fpmc.hip): the slot sampler and the fused forward / backward over 5 + c rows
def fpmc_geometry():
    """(max_window, max_rank, rank_multiple): the most context items an event takes; fpmc_fwd_bwd takes a rank that is a
    multiple of rank_multiple and at most max_rank."""
    return _geometry("fpmc", 3)


def fpmc_sample(seq_offsets, seq_upos, seq_ipos, row_offsets, row_ipos, nu, ni, window, seed, step0, K, B):
    """K steps of B slots drawn on the device: (u, e, c, i, j, valid) int32 [K, B] -- row k is global step step0 + k (mod
    2^32) -- and dropped int32[K], the count of valid == 0 per step.  The sequences are a CSR by user in time order on the
    DEVICE (seq_offsets int64[nu + 1], seq_upos / seq_ipos int32[nnz_seq], repeats kept), the seen pairs bpr_sample's CSR
    (row_offsets int64[nu + 1], row_ipos int32[nnz_seen]).  The rule is esr_fpmc_sample.h's: e is the event, i its item,
    c = min(place in u's sequence, window) its context length, j bpr_sample's negative."""
    lib = _lib.load()
    nu, ni, K, B, window = int(nu), int(ni), int(K), int(B), int(window)
    nnz_seq = _check_device_csr("fpmc_sample", "seq_offsets", seq_offsets, seq_upos, seq_ipos, nu, ni=ni, K=K, B=B)
    _req(row_offsets, torch.int64, "row_offsets"), _req(row_ipos, torch.int32, "row_ipos")
    nnz_seen = row_ipos.numel()
    if row_offsets.numel() != nu + 1 or not 1 <= nnz_seen <= 2 ** 31 - 1:
        raise ValueError("fpmc_sample: row_offsets holds %d entries for nu = %d, row_ipos %d pairs (in [1, 2^31 - 1])"
                         % (row_offsets.numel(), nu, nnz_seen))
    if not 1 <= window <= fpmc_geometry()[0]:
        raise ValueError("fpmc_sample: window = %d outside [1, %d]" % (window, fpmc_geometry()[0]))
    out, dropped = _sample_outputs(6, K, B, seq_upos.device)
    check(lib.esr_fpmc_sample(_p(seq_offsets), _p(seq_upos), _p(seq_ipos), nnz_seq, _p(row_offsets), _p(row_ipos), nnz_seen,
                              nu, ni, window, int(seed) & (2 ** 64 - 1), int(step0) & 0xFFFFFFFF, K, B, _p(out[0]),
                              _p(out[1]), _p(out[2]), _p(out[3]), _p(out[4]), _p(out[5]), _p(dropped), _stream()),
          "esr_fpmc_sample")
    return out[0], out[1], out[2], out[3], out[4], out[5], dropped


def fpmc_fwd_bwd(user_table, item_table, next_table, prev_table, seq_ipos, u, e, c, i, j, valid, reg, ctx_offsets=None,
                 M=None, want_grads=True, want_diff=False, failed=None):
    """(loss_t float32[B], diff_t float32[B] or None, grads float32[5 B + M, D] or None, ctx_ids int32[M] or None) of the
    slots (u, e, c, i, j) int32[B] of fpmc_sample over the tables U [nu, D] and A, Bn, P [ni, D]:
    d = U_u . (A_i - A_j) + m . (Bn_i - Bn_j), m the bag of the c items before event e (seq_ipos[e - c .. e - 1], weight
    1 / c each), loss_t = softplus(-d), diff_t = d, and the gradient rows [U ; A_i ; A_j ; Bn_i ; Bn_j ; context
    occurrences] in occurrence order with the L2 term reg * row (include/esr_hip.h); ctx_ids names the P row of every
    context occurrence.  ctx_offsets int64[B + 1] is the exclusive scan of c and M its last entry (both computed here,
    with one host read, when None).  valid int32[B] or None (all valid): valid = 0 gives zeros under the real ctx_ids.
    `failed` (int32[1], device; a scratch word when None) gets bit 30 when a position lies outside its table or a slot's
    (e, c) does not stand -- that slot gives zeros; the caller zeroes and reads it."""
    lib = _lib.load()
    tables = (user_table, item_table, next_table, prev_table)
    for t, name in zip(tables, ("user_table", "item_table", "next_table", "prev_table")):
        _req(t, torch.float32, name)
    if any(t.dim() != 2 for t in tables) or len({int(t.shape[1]) for t in tables}) != 1 or \
            not item_table.shape == next_table.shape == prev_table.shape:
        raise ValueError("user_table [nu, rank] and item_table, next_table, prev_table [ni, rank] must share one rank")
    _req(seq_ipos, torch.int32, "seq_ipos")
    ids = (u, e, c, i, j)
    for t, name in zip(ids, "uecij"):
        _req(t, torch.int32, name)
    B, D = u.numel(), int(user_table.shape[1])
    if any(t.numel() != B for t in ids):
        raise ValueError("u, e, c, i and j must have one length")
    _check_valid(valid, B, "slot")
    _check_rank4(D, *fpmc_geometry()[1:])
    dev = user_table.device
    failed = _failed_word(failed, dev)
    ctx_ids = None
    if want_grads:
        if ctx_offsets is None:
            ctx_offsets = torch.zeros(B + 1, dtype=torch.int64, device=dev)
            torch.cumsum(c.reshape(-1), 0, out=ctx_offsets[1:])
            M = int(ctx_offsets[-1]) if B else 0
        _req(ctx_offsets, torch.int64, "ctx_offsets")
        M = int(M)
        if ctx_offsets.numel() != B + 1 or not 0 <= M <= 2 ** 31 - 1:
            raise ValueError("fpmc_fwd_bwd: ctx_offsets must hold B + 1 entries and M = %d lie in [0, 2^31 - 1]" % M)
        ctx_ids = torch.empty(M, dtype=torch.int32, device=dev)
    loss_t, diff_t, grads = _step_outputs(B, 5 * B + (M or 0), D, dev, want_grads, want_diff)
    if B:
        check(lib.esr_fpmc_fwd_bwd(_p(user_table), user_table.shape[0], _p(item_table), _p(next_table), _p(prev_table),
                                   item_table.shape[0], D, _p(seq_ipos), seq_ipos.numel(), _p(u), _p(e), _p(c), _p(i), _p(j),
                                   _p(valid), B, _p(ctx_offsets) if want_grads else 0, M if want_grads else 0, float(reg),
                                   _p(loss_t), _p(diff_t), _p(grads), _p(ctx_ids) if want_grads and M else 0, _p(failed),
                                   _stream()), "esr_fpmc_fwd_bwd")
    return loss_t, diff_t, grads, ctx_ids


# ---------------------------------------------------------------------------------------------
# Skip-gram with negative sampling (esr_sgns.hip): the slot sampler and the fused forward / backward over 2 + K rows
def sgns_geometry():
    """(max_window, max_negatives, max_rank, rank_multiple): the largest context distance and the most noise items per
    slot; sgns_fwd_bwd takes a rank that is a multiple of rank_multiple and at most max_rank."""
    return _geometry("sgns", 4)


def sgns_sample(seq_offsets, seq_upos, seq_ipos, nd, ni, window, negatives, noise_keep, noise_alias, seed, step0, K, B):
    """K steps of B slots drawn on the device: (c, e, o, valid) int32 [K, B], neg int32 [K, B, negatives] -- row k is
    global step step0 + k (mod 2^32) -- and dropped int32[K], the count of valid == 0 per step.  The documents are a CSR in
    order on the DEVICE (seq_offsets int64[nd + 1], seq_upos / seq_ipos int32[nnz_seq], repeats kept); the noise table is
    noise_keep (the uint32 thresholds, held as int32 bits) and noise_alias int32[ni].  The rule is esr_sgns_sample.h's:
    e is the event, c its item, o the item at a distance d <= window drawn with weight window - d + 1 on a random side
    (valid = 0 where that leaves the document), neg the alias table's draws."""
    lib = _lib.load()
    nd, ni, K, B, window, negatives = int(nd), int(ni), int(K), int(B), int(window), int(negatives)
    nnz_seq = _check_device_csr("sgns_sample", "seq_offsets", seq_offsets, seq_upos, seq_ipos, nd, ni=ni, K=K, B=B)
    _req(noise_keep, torch.int32, "noise_keep"), _req(noise_alias, torch.int32, "noise_alias")
    if noise_keep.numel() != ni or noise_alias.numel() != ni:
        raise ValueError("sgns_sample: noise_keep and noise_alias must hold ni = %d entries" % ni)
    top_window, top_negatives = sgns_geometry()[:2]
    if not 1 <= window <= top_window:
        raise ValueError("sgns_sample: window = %d outside [1, %d]" % (window, top_window))
    if not 1 <= negatives <= top_negatives:
        raise ValueError("sgns_sample: negatives = %d outside [1, %d]" % (negatives, top_negatives))
    dev = seq_upos.device
    out, dropped = _sample_outputs(4, K, B, dev)
    neg = torch.empty((K, B, negatives), dtype=torch.int32, device=dev)
    check(lib.esr_sgns_sample(_p(seq_offsets), _p(seq_upos), _p(seq_ipos), nnz_seq, nd, ni, window, negatives, _p(noise_keep),
                              _p(noise_alias), int(seed) & (2 ** 64 - 1), int(step0) & 0xFFFFFFFF, K, B, _p(out[0]), _p(out[1]),
                              _p(out[2]), _p(out[3]), _p(neg), _p(dropped), _stream()), "esr_sgns_sample")
    return out[0], out[1], out[2], out[3], neg, dropped


def sgns_fwd_bwd(in_table, out_table, c, o, neg, valid, reg, want_grads=True, want_diff=False, failed=None):
    """(loss_t float32[B], diff_t float32[B, 1 + K] or None, grads float32[(2 + K) B, D] or None) of the slots (c, o)
    int32[B], neg int32[B, K] over the tables in [ni, D] (centre vectors) and out [ni, D] (context vectors):
    s_o = v_c . w_o, s_k = v_c . w_{n_k}, m_k = (n_k != o), loss_t = softplus(-s_o) + sum_k m_k softplus(s_k), diff_t =
    [s_o, s_0, ..], and the gradient rows [centre ; positive ; noise k-major] in occurrence order with the L2 term
    reg * row (include/esr_hip.h).  valid int32[B] or None (all valid): valid = 0 gives zeros.  `failed` (int32[1], device;
    a scratch word when None) gets bit 30 when an id lies outside the tables -- that slot gives zeros too; the caller
    zeroes and reads it."""
    lib = _lib.load()
    _req(in_table, torch.float32, "in_table"), _req(out_table, torch.float32, "out_table")
    _req(c, torch.int32, "c"), _req(o, torch.int32, "o"), _req(neg, torch.int32, "neg")
    if in_table.dim() != 2 or in_table.shape != out_table.shape:
        raise ValueError("in_table and out_table must be [ni, rank] alike")
    B, D = c.numel(), int(in_table.shape[1])
    if neg.dim() != 2 or o.numel() != B or neg.shape[0] != B:
        raise ValueError("c and o must have one length B and neg be [B, negatives]")
    K = int(neg.shape[1])
    if not 1 <= K <= sgns_geometry()[1]:
        raise ValueError("sgns_fwd_bwd: negatives = %d outside [1, %d]" % (K, sgns_geometry()[1]))
    _check_valid(valid, B, "slot")
    _check_rank4(D, *sgns_geometry()[2:])
    dev = in_table.device
    failed = _failed_word(failed, dev)
    loss_t, diff_t, grads = _step_outputs(B, (2 + K) * B, D, dev, want_grads, want_diff, scores=1 + K)
    if B:
        check(lib.esr_sgns_fwd_bwd(_p(in_table), _p(out_table), in_table.shape[0], D, _p(c), _p(o), _p(neg), _p(valid), B, K,
                                   float(reg), _p(loss_t), _p(diff_t), _p(grads), _p(failed), _stream()), "esr_sgns_fwd_bwd")
    return loss_t, diff_t, grads


# ---------------------------------------------------------------------------------------------
# Diversity re-ranking (esr_rerank.hip): MMR over candidate lists, intra-list similarity
def rerank_geometry(D, width):
    """A dict for lists of `width` candidates over rows of rank `D`: the limits (max_rank, rank_multiple, max_width,
    max_cutoffs), the staging budget stage_bytes, the grid_cap, whether this shape stages a query's rows in LDS (staged)
    and the dynamic LDS of its launch (lds_bytes)."""
    names = ("max_rank", "rank_multiple", "max_width", "max_cutoffs", "stage_bytes", "grid_cap", "staged", "lds_bytes")
    vals = [ctypes.c_int(0) for _ in names]
    check(_lib.load().esr_rerank_geometry(int(D), int(width), *[ctypes.byref(v) for v in vals]), "esr_rerank_geometry")
    return {n: int(v.value) for n, v in zip(names, vals)}


def _rerank_args(who, rows, cand, lengths):
    """The checks rerank_mmr and rerank_ils share.  Returns (ni, D, nq, width)."""
    _req(rows, torch.float32, "rows"), _req(cand, torch.int32, "cand")
    if rows.dim() != 2 or cand.dim() != 2:
        raise ValueError("%s: rows must be [ni, rank] and cand [nq, width]" % who)
    ni, D, nq, width = int(rows.shape[0]), int(rows.shape[1]), int(cand.shape[0]), int(cand.shape[1])
    _check_rank4(D, 128, 4)
    if not 1 <= width <= 1024:
        raise ValueError("%s: list width = %d outside [1, 1024]" % (who, width))
    if not (1 <= ni <= 2 ** 31 - 1 and nq <= 2 ** 31 - 1):
        raise ValueError("%s: ni=%d nq=%d (ni in [1, 2^31 - 1], nq at most 2^31 - 1)" % (who, ni, nq))
    if lengths is not None:
        _req(lengths, torch.int32, "lengths")
        if lengths.numel() != nq:
            raise ValueError("%s: lengths must hold one entry per query" % who)
    return ni, D, nq, width


def rerank_mmr(rows, cand, rel, lengths, lam, n_out, failed=None):
    """(out_pos int32, out_item int32, out_rel float32, out_value float32 [nq, n_out], out_length int32[nq]): n_out greedy
    rounds of Maximal Marginal Relevance per query by the rule of esr_rerank_rule.h over cand int32[nq, width] (item
    positions into rows float32[ni, D]), rel float32[nq, width] and lengths int32[nq] or None (full rows): round t picks
    the candidate with the greatest fmaf(lam, rel, -((1 - lam) * m)), m its greatest dot product with a row picked before,
    ties to the smallest list position.  `failed` (int32[1], device; a scratch word when None) gets bit 30 for a position
    outside rows and bit 29 for a rel that is not finite -- such a candidate is never picked; the caller zeroes and reads
    it."""
    lib = _lib.load()
    ni, D, nq, width = _rerank_args("rerank_mmr", rows, cand, lengths)
    _req(rel, torch.float32, "rel")
    if rel.shape != cand.shape:
        raise ValueError("rerank_mmr: rel must have cand's shape")
    n_out, lam = int(n_out), float(lam)
    if not 1 <= n_out <= width:
        raise ValueError("rerank_mmr: n_out = %d outside [1, width = %d]" % (n_out, width))
    if not 0.0 <= lam <= 1.0:
        raise ValueError("rerank_mmr: lam = %r outside [0, 1]" % lam)
    dev = rows.device
    out_pos = torch.empty((nq, n_out), dtype=torch.int32, device=dev)
    out_item, out_rel = torch.empty_like(out_pos), torch.empty((nq, n_out), dtype=torch.float32, device=dev)
    out_value, out_length = torch.empty_like(out_rel), torch.empty(nq, dtype=torch.int32, device=dev)
    failed = _failed_word(failed, dev)
    if nq:
        check(lib.esr_rerank_mmr(_p(rows), ni, D, _p(cand), _p(rel), _p(lengths), nq, width, n_out, lam, _p(out_pos),
                                 _p(out_item), _p(out_rel), _p(out_value), _p(out_length), _p(failed), _stream()),
              "esr_rerank_mmr")
    return out_pos, out_item, out_rel, out_value, out_length


def rerank_ils(rows, cand, lengths, ks, failed=None):
    """(ils float32[nq, nk], valid int32[nq, nk]): the intra-list similarity of the lists cand int32[nq, width] (item
    positions into rows float32[ni, D]; lengths int32[nq] or None) at the strictly ascending cutoffs `ks` (1 to 8 ints):
    the mean dot product over the pairs among a list's first min(k, length) candidates, summed in fp64 in a fixed order;
    0 with valid = 0 for fewer than two candidates.  `failed` as rerank_mmr's (bit 30 only)."""
    lib = _lib.load()
    ni, D, nq, width = _rerank_args("rerank_ils", rows, cand, lengths)
    try:
        ks = tuple(int(k) for k in ks)
    except TypeError:
        raise TypeError("ks must be a sequence of ints, got %r" % (ks,))
    if not 1 <= len(ks) <= 8:
        raise ValueError("ks holds %d cutoffs, outside [1, 8]" % len(ks))
    if any(k < 1 or k > 2 ** 31 - 1 or (j and k <= ks[j - 1]) for j, k in enumerate(ks)):
        raise ValueError("ks must be strictly ascending cutoffs >= 1, got %r" % (ks,))
    dev = rows.device
    ils = torch.empty((nq, len(ks)), dtype=torch.float32, device=dev)
    valid = torch.empty((nq, len(ks)), dtype=torch.int32, device=dev)
    failed = _failed_word(failed, dev)
    if nq:
        check(lib.esr_rerank_ils(_p(rows), ni, D, _p(cand), _p(lengths), nq, width, (ctypes.c_int32 * len(ks))(*ks), len(ks),
                                 _p(ils), _p(valid), _p(failed), _stream()), "esr_rerank_ils")
    return ils, valid
