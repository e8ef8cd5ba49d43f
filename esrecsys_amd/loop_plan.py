"""Host side of the epoch loops' look-ahead (pinterest.train_steps / presorted, wikipedia.train_epoch): long-run hints
that kernels write straight into pinned host memory, and the planner that sorts and plans a group of coming batches
while the group before it is stepped.

A step needs its long-run launch only when an id of its occurrence list has a run longer than a 32-position chunk.  The
kernel that sees the sorted list (a plan kernel, or esr_long_run_hint) stores a GENERATION number into a hint word when
it finds such a run and nothing otherwise, so a word is never cleared: it says "long" exactly when it equals the
generation of the launch that was asked.  The word is valid on the host once an event recorded behind the launch has
completed.  A lost hint costs speed only -- the step makes its long-run launch, the tables stay bit-identical -- so only a
launch count shows a mistake here (tests/test_gpu_loop_launches.py).
"""
import ctypes

import torch

from . import _lib, ops

_hint_ring = {}  # device -> [pinned int32 [R], next slot, next gen]
_hint_owner = {}  # address of a ring word -> the generation it was last handed to


def _hint_slot(dev):
    """One word of a small ring of PINNED host memory for a long-run hint: (view [1], gen).  The kernels write the word
    themselves (pinned memory is mapped into the device's address space): no copy launch."""
    R = 16
    key = (dev.type, dev.index)
    if key not in _hint_ring:
        _hint_ring[key] = [torch.zeros(R, dtype=torch.int32).pin_memory(), 0, 1]
    ring = _hint_ring[key]
    i, gen = ring[1], ring[2]
    ring[1], ring[2] = (i + 1) % R, gen + 1 if gen < 2 ** 31 - 2 else 1
    word = ring[0][i:i + 1]
    _hint_owner[word.data_ptr()] = gen  # the slot is this generation's until the ring comes round to it again
    return word, gen


def hint_value(hint):
    """1 / 0 = the hint kernel of `hint` = (word, gen, ...) found / did not find a long run -- valid only while the word
    is still this generation's.  A kernel writes its gen into the word only when it finds a long run, so a word that a
    LATER hint has been handed (more than a ring's worth of handles outstanding) would read as "no long run" whatever
    this generation's kernel had found: that case answers -1 (unknown: the step makes its long-run launch)."""
    word, gen = hint[0], hint[1]
    if _hint_owner.get(word.data_ptr()) != gen:
        return -1
    return 1 if int(word[0]) == gen else 0


def hint_long_runs(hint):
    """A step's ``long_runs`` from `hint` = (word, gen, event recorded behind the hint's launch) or None: 0 / 1 once
    the hint has reached the host, -1 while nobody knows (the step then makes its long-run launch)."""
    if hint is None or not hint[2].query():
        return -1
    return hint_value(hint)


def screen_group(sorted_ids, dev):
    """One screening launch on the current stream for a whole group of sorted lists ([nb, n] taken as ONE list: a run
    across two lists can only make the answer "long"): the (word, gen, event) hint every step of the group shares."""
    word, gen = _hint_slot(dev)
    ops.long_run_hint(sorted_ids.reshape(-1), 32, word, gen)
    event = torch.cuda.Event()
    event.record()
    return word, gen, event


class Group:
    """A group of batches whose id lists were sorted and planned together (GroupPlanner.plan): the raw pointers a
    trainer's group call takes, and the tensors behind them, kept alive."""
    __slots__ = "nb", "B", "ptrs", "tgt_ptrs", "sorted_ptr", "perm_ptr", "plans_ptr", "which", "gen", "keep", "side", "long"

    def __init__(self, nb, B, ptrs, tgt_ptrs, sorted_ptr, perm_ptr, plans_ptr, which, gen, keep, side):
        self.nb, self.B, self.ptrs, self.tgt_ptrs = nb, B, ptrs, tgt_ptrs
        self.sorted_ptr, self.perm_ptr, self.plans_ptr = sorted_ptr, perm_ptr, plans_ptr
        self.which, self.gen, self.keep = which, gen, keep  # keep: the id (and target) tensors, alive
        self.side = side  # sorted + planned on a second stream: the group's first step waits for its event
        self.long = None  # GroupPlanner.long_runs' answer once the host has it: per-step callers index it


class GroupPlanner:
    """Sorts and plans up to `max_group` coming batches by one call pair (esr_segment_sort_ids_batched + the trainer's
    plan entry point) into one of two buffer sets, so that group g + 1 is made while group g steps.  The plan kernel
    writes one hint word per batch into pinned memory (`words[which]`, the call's generation where the list has a long
    run) and an event is recorded behind it; ``long_runs`` turns the words into the steps' ``long_runs`` values once the
    host has seen that event complete.  With `hint_wait` the host waits for it: the launch was queued in front of the
    steps of the group before, so the wait ends with a group's worth of work still queued -- the device never runs dry,
    the host stays at most two groups ahead, and every step knows whether it needs its long-run launch (a loop that ran
    further ahead never saw a hint in time and made all of them: 4.8 us per step at 8192 triplets).  segs: id segments
    per list (3 for triplets; 1 for GloVe's [2, B] inputs, which carry a target array per list as well)."""

    def __init__(self, dev, max_group, hint_wait, segs, targets=False):
        self.dev, self.max, self.hint_wait, self.segs = dev, max_group, hint_wait, segs
        self.lib, self.check = _lib.load(), _lib.check
        # (kept arrays: ops.segment_sort_batched re-validates every tensor and rebuilds its ctypes arrays, 67 us per group)
        self.ptrs = [(ctypes.c_void_p * (segs * max_group))() for _ in range(2)]
        self.tgt_ptrs = [(ctypes.c_void_p * max_group)() if targets else None for _ in range(2)]
        self.bufs = {}  # (set, with plan records?) -> sorted ids, perm, batched-sort workspace, plan records or None
        self.words = torch.zeros((2, max_group), dtype=torch.int32).pin_memory()
        self.events = [torch.cuda.Event(), torch.cuda.Event()]
        self.known = [None, None]  # per set: its words as a list once the event has been seen complete
        self.long_arr = [(ctypes.c_int32 * max_group)() for _ in range(2)]
        self.gen = 0

    def buffers(self, which, n, plan_bytes=0):
        """Set `which` for lists of n ids: (sorted ids, perm, batched-sort workspace, plan records -- room for plan_bytes
        per list, None without) as [max_group, ...] tensors, reallocated when the list length changes (sets with and
        without plan records are kept apart: an epoch that mixes both reallocates neither).  New plan records are zeroed
        by a launch on the CURRENT stream: a caller that plans on another stream calls this in front of the hand-over."""
        key = (which, plan_bytes > 0)
        buf = self.bufs.get(key)
        if buf is None or buf[0].shape[1] != n:
            buf = self.bufs[key] = (
                torch.empty((self.max, n), dtype=torch.int32, device=self.dev),
                torch.empty((self.max, n), dtype=torch.int32, device=self.dev),
                ops._ws(ops._ws_bytes("esr_segment_sort_batched_workspace_bytes", n, self.max), self.dev),
                ops._aligned_bytes(self.max * plan_bytes, self.dev) if plan_bytes else None)
        return buf

    def sort(self, which, nb, bufs, lists, raw):
        """The nb lists whose segment pointers stand in ``ptrs[which]`` (lists = (counts, offsets, rows) of their
        segments) sorted by ONE call on stream `raw` into `bufs` (``buffers`` of set `which`)."""
        srt, prm, ws, _ = bufs
        cnt, off, rows = lists
        self.check(self.lib.esr_segment_sort_ids_batched(self.ptrs[which], cnt, off, self.segs, nb, rows, srt.data_ptr(),
                                                         prm.data_ptr(), ws.data_ptr(), ws.numel(), raw),
                   "esr_segment_sort_ids_batched")

    def plan(self, which, nb, B, bufs, lists, plan, keep, stream=None, side=False):
        """``sort`` and then the plan call, `plan` = (the library's entry point, its arguments in front of ``sorted,
        perm, plans, hint words, generation, stream``), on `stream` (default: the current one) under a new generation;
        the set's event is recorded behind them and what was known of the set's words forgotten.  Returns the Group."""
        raw = ops._stream() if stream is None else stream.cuda_stream
        self.sort(which, nb, bufs, lists, raw)
        srt, prm, _, plans = bufs
        self.gen += 1
        plan_fn, args = plan
        self.check(plan_fn(*args, srt.data_ptr(), prm.data_ptr(), plans.data_ptr(), self.words[which].data_ptr(),
                           self.gen, raw), plan_fn.__name__)
        if stream is None:
            self.events[which].record()
        else:
            self.events[which].record(stream)
        self.known[which] = None
        return Group(nb, B, self.ptrs[which], self.tgt_ptrs[which], srt.data_ptr(), prm.data_ptr(), plans.data_ptr(),
                     which, self.gen, keep, side)

    def long_runs(self, gr):
        """The ``long_runs`` values of group `gr`'s steps as a c_int32 array (1: the batch's word is the group's
        generation; 0: anything else, a later generation's included), also left in ``gr.long`` for per-step callers
        ([j] is batch j's; -1 while there is none) -- or None when the host has not seen the set's event complete: the
        library then makes every long-run launch, and a group planned on a second stream is waited for on the device."""
        known = self.known[gr.which]
        if known is None:
            event = self.events[gr.which]
            if self.hint_wait:
                event.synchronize()
            if not event.query():
                return None
            known = self.known[gr.which] = self.words[gr.which].tolist()
        long_runs, gen = self.long_arr[gr.which], gr.gen
        for j in range(gr.nb):
            long_runs[j] = 1 if known[j] == gen else 0
        gr.long = long_runs
        return long_runs
