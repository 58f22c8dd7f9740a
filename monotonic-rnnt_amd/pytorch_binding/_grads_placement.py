"""Placement-aware gradient buffers for large calls.

On MI355X the streaming write rate of a large allocation depends on its physical backing: about one in three
52.7 GB grads buffers of the headline writes ~20 % slower than the others (5.2-5.5 against 6.5-7.2 TB/s for a
nontemporal fill of the whole buffer; gradient pass 15.3-16.0 against 12.4-13.1 ms). The counters put it on the
memory side -- 2.5x the DRAM write-credit stalls, same address-translation traffic
(profiles/r02/slow_buffer/rootcause_pmc.json) -- and the rate is constant over the buffer's life, so the caching
allocator, which hands the same block to every later step, keeps a slow draw for the whole run.

For gradient outputs of at least MIN_BYTES this module keeps one buffer per (device, dtype), chosen once: a
candidate from the caching allocator is timed with one nontemporal zero fill over its whole length
(mrnnt_fill_zero, the gradient pass's store stream: ~8 ms for 52.7 GB); below FAST_GBPS ONE further candidate is
allocated while the first is still held (so it is a different block) when free memory allows (>= 3x the need),
and the faster is kept; the other candidate is released to the driver (torch.cuda.empty_cache), so the caching
allocator holds no second block of that size.

Reuse is safe by construction: the kept buffer is only ever caching-allocator memory, and it goes back through the
allocator at every reuse. Each call hands out a view of the kept storage; on the next call, if nothing else holds
it (storage use count 1: the caller dropped the previous gradient), the module drops its own reference -- the
allocator then honours every stream the caller recorded on it (Tensor.record_stream: the block is not reusable
until those streams pass their events) -- and immediately asks the allocator for the same size on the current
stream. When the block is ready the allocator's best fit returns that very block (a "hit": the fast placement is
kept); when a side stream still uses it, or the stream differs, it returns another block (a "miss", counted): that
block is handed out as a plain allocation -- not kept, so the caching allocator gets it back when the caller drops
the gradient, and the module never holds a second block of that size -- and the next call tries to take the fast
block back again (after two misses in a row it gives up on it and chooses afresh). A gradient the caller still
holds is never reused (plain allocation). Under HIP-graph
capture the graph's memory pool serves gradients as usual. MRNNT_GRADS_PLACEMENT=0 turns this off (plain
torch.empty_like), and so does a torch without the storage use count; release() drops the kept buffers.

Row state. The kept block is written by the library itself, step after step, and about half of a
gradient's rows are exact zeros (out of band, or dead). like_tracked() therefore hands out, beside the buffer, a
ticket with one state byte per row (0 unknown, 1 all +0.0, 2 all -0.0) for mrnnt_backward_tracked /
mrnnt_path_backward_tracked, which skip the store of a row that already holds the zero it would get and leave the
state describing what the buffer holds now. The arena vouches for the state of the previous step only when it can
prove that nothing but that tracked launch wrote the block since:
  * the hand-out is a hit (the allocator returned the kept block itself) on the stream of the last tracked launch;
  * the previous hand-out was committed (ticket.commit(): the tracked launch was enqueued) -- an exception before the
    launch, or a backward through the untracked entry (like()), leaves it uncommitted;
  * the row size (bytes) is the one the state was built for;
  * nobody wrote through torch: the arena keeps a detach() alias of the tensor it handed out -- same storage, same
    version counter, another TensorImpl, so autograd still takes the gradient without a copy -- and the alias's
    _version is unchanged (in-place ops through .grad, a view, out= or under no_grad all bump it);
  * nobody else was handed the block between the arena dropping its references and getting it back: the allocator's
    allocation counter moved by exactly one over that window. After a miss the block sat in the allocator for a
    whole step, so the state is dropped.
In every other case the ticket carries a newly allocated all-zero state (never an in-place reset: the old tensor may
still be read on another stream) and the kernel writes every row; a plain allocation (bypass, held, miss) has no
ticket and takes the untracked entry. ONE HOLE REMAINS: a write that does not go through torch's version counter --
`.data`, or a foreign kernel given the raw pointer -- is invisible, exactly as it is to autograd's own saved-tensor
check (which MonotonicRNNTFunction.forward already relies on for acts). Whoever writes a gradient that way must call
forget() (or release()) before the next backward.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Callable, Dict, List, Optional, Tuple

import torch

MIN_BYTES = 4 << 30        # below this a slow draw costs under a millisecond: plain allocations
FAST_GBPS = 6300.0         # whole-buffer nontemporal fill rate of the fast classes (6.5-7.2 TB/s measured)
MAX_CANDIDATES = 2         # the first draw and at most one more
FREE_FACTOR = 3            # a further candidate only while free memory is >= FREE_FACTOR x its size


# storage use count (private torch API, present in 2.x): without it a kept buffer could not be proven unshared,
# so the module falls back to plain allocations
_use_count = getattr(torch._C, "_storage_Use_Count", None)


def enabled() -> bool:
    return _use_count is not None and os.environ.get("MRNNT_GRADS_PLACEMENT", "1") != "0"


class _Kept:
    """The kept block (storage held), or -- after a missed take-back -- only its record (storage None): the block sits
    in the caching allocator until the streams recorded on it pass, and the next call asks for it again."""
    __slots__ = ("storage", "ptr", "nbytes", "gbps", "misses")

    def __init__(self, storage, nbytes: int, gbps: Optional[float], ptr: Optional[int] = None, misses: int = 0):
        self.storage, self.nbytes, self.gbps, self.misses = storage, nbytes, gbps, misses
        self.ptr = storage.data_ptr() if storage is not None else ptr


def _fill_gbps(buf: torch.Tensor) -> float:
    """Time one whole-buffer nontemporal zero fill (after one untimed fill) on the current stream."""
    try:
        from . import _mrnnt_lib as L
    except ImportError:
        import _mrnnt_lib as L
    n = buf.numel() - buf.numel() % 16
    stream = torch.cuda.current_stream(buf.device)
    sp = ctypes.c_void_p(stream.cuda_stream)
    fill = L.load().mrnnt_fill_zero
    L.check(fill(ctypes.c_void_p(buf.data_ptr()), n, sp), "fill_zero")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    L.check(fill(ctypes.c_void_p(buf.data_ptr()), n, sp), "fill_zero")
    e1.record(stream)
    e1.synchronize()
    return n / (e0.elapsed_time(e1) * 1e-3) / 1e9


def _free_bytes(dev: torch.device) -> int:
    free, _ = torch.cuda.mem_get_info(dev)
    return int(free)


def _alloc_count(dev: torch.device) -> Optional[int]:
    """Allocations the caching allocator has served on `dev` so far (cumulative), or None when it cannot be told."""
    if dev.type != "cuda":
        return None
    try:
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        return int(torch._C._cuda_memoryStats(idx)["allocation"]["all"]["allocated"])
    except Exception:  # a torch without the private accessor: the public, slower one
        try:
            return int(torch.cuda.memory_stats(dev)["allocation.all.allocated"])
        except Exception:
            return None


def _version_of(t: torch.Tensor) -> Optional[int]:
    try:
        return int(t._version)
    except Exception:  # (an inference tensor keeps no version counter: never vouched for)
        return None


def _stream_of(dev: torch.device) -> int:
    return int(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else 0


class _Track:
    """What the arena knows about the contents of the kept block of one (device, dtype)."""
    __slots__ = ("state", "row_bytes", "alias", "version", "committed", "stream")

    def __init__(self, state: torch.Tensor, row_bytes: int):
        self.state, self.row_bytes = state, row_bytes
        self.alias, self.version, self.committed, self.stream = None, -1, False, None


class Ticket:
    """Handed out with a tracked buffer: `state` goes to the tracked backward entry; commit() once it is enqueued."""
    __slots__ = ("state", "vouched", "_arena", "_key", "_track")

    def __init__(self, arena: "GradsArena", key, track: _Track, vouched: bool):
        self.state, self.vouched, self._arena, self._key, self._track = track.state, vouched, arena, key, track

    def commit(self) -> None:
        a = self._arena
        with a._lock:
            if a._track.get(self._key) is self._track:
                self._track.committed = True
                self._track.stream = a._stream_of(self._key[0])


class GradsArena:
    """One kept gradient buffer per (device, dtype). The device hooks are injectable for host-side tests."""

    def __init__(self, probe: Callable[[torch.Tensor], float] = _fill_gbps,
                 free_bytes: Callable[[torch.device], int] = _free_bytes,
                 alloc: Optional[Callable[[int, torch.device], torch.Tensor]] = None,
                 release_unused: Optional[Callable[[], None]] = None,
                 fast_gbps: float = FAST_GBPS, max_candidates: int = MAX_CANDIDATES, min_bytes: int = MIN_BYTES,
                 require_cuda: bool = True, allocator_refs: int = 0,
                 on_release: Optional[Callable[[int], None]] = None,
                 alloc_count: Callable[[torch.device], Optional[int]] = _alloc_count,
                 stream_of: Callable[[torch.device], int] = _stream_of):
        self._probe, self._free = probe, free_bytes
        self._alloc = alloc or (lambda n, dev: torch.empty(n, dtype=torch.uint8, device=dev))
        self._release_unused = release_unused or (lambda: torch.cuda.empty_cache())
        self.fast_gbps, self.max_candidates, self.min_bytes = fast_gbps, max_candidates, min_bytes
        self.require_cuda = require_cuda
        self._on_release = on_release  # test hook: told the address of every block this arena lets go of
        self._held = 1 + allocator_refs  # storage references when only this arena holds the block (a test
        #                                 allocator may keep one of its own)
        self._alloc_count, self._stream_of = alloc_count, stream_of
        self._kept: Dict[Tuple[torch.device, torch.dtype], _Kept] = {}
        self._track: Dict[Tuple[torch.device, torch.dtype], _Track] = {}  # row state of the kept blocks
        self._lock = threading.Lock()
        self.log: List[dict] = []  # one record per placement decision (bench.py reports it)
        self.stats = {"handed_out": 0, "reuse_hits": 0, "reuse_misses": 0, "held_by_caller": 0}
        self.track_stats = {"tickets": 0, "vouched": 0}

    def like(self, acts: torch.Tensor) -> torch.Tensor:
        """A contiguous uninitialised tensor of acts' shape, dtype and device (its contents are not tracked)."""
        return self._hand_out(acts, None)[0]

    def like_tracked(self, acts: torch.Tensor, row_elems: Optional[int] = None) -> Tuple[torch.Tensor, Optional[Ticket]]:
        """like(), and for the kept block a Ticket with the row state (rows of row_elems elements, default acts' last
        dimension); None with a plain allocation, which takes the untracked backward."""
        row_elems = int(acts.shape[-1]) if row_elems is None else int(row_elems)
        return self._hand_out(acts, max(1, row_elems) * acts.element_size())

    def forget(self) -> None:
        """Somebody wrote a handed-out gradient behind torch's back (`.data`, a raw pointer): vouch for nothing."""
        with self._lock:
            self._drop_tracks()

    def _drop_tracks(self, key=None) -> None:
        """Forget the row state of `key` (None: of every kept block); its alias must not keep the block alive."""
        for k in ([key] if key is not None else list(self._track)):
            t = self._track.pop(k, None)
            if t is not None:
                t.alias = None

    def _ticket(self, key, out: torch.Tensor, row_bytes: Optional[int], kb: int, vouch: bool) -> Optional[Ticket]:
        """The row state that goes with `out`, a view of the kept block of `key` (kb bytes), handed out now."""
        t = self._track.pop(key, None)
        if t is not None:
            t.alias = None
        if row_bytes is None:
            return None  # an untracked hand-out: nothing is known about the block afterwards
        stream = self._stream_of(key[0])
        vouch = (vouch and t is not None and t.row_bytes == row_bytes and t.stream == stream
                 and t.state.numel() >= kb // row_bytes)
        if not vouch:  # a new all-zero state, never an in-place reset (the old one may still be read elsewhere)
            t = _Track(torch.zeros(max(1, kb // row_bytes), dtype=torch.uint8, device=key[0]), row_bytes)
        t.committed, t.stream = False, None
        t.alias = out.detach()  # shares storage and version counter with what the caller gets
        t.version = _version_of(t.alias)
        self._track[key] = t
        self.track_stats["tickets"] += 1
        self.track_stats["vouched"] += int(vouch)
        return Ticket(self, key, t, vouch)

    def _hand_out(self, acts: torch.Tensor, row_bytes: Optional[int]) -> Tuple[torch.Tensor, Optional[Ticket]]:
        nbytes = acts.numel() * acts.element_size()
        if nbytes < self.min_bytes or (self.require_cuda and not acts.is_cuda) or _capturing(acts):
            return torch.empty_like(acts, memory_format=torch.contiguous_format), None
        key = (acts.device, acts.dtype)
        with self._lock:
            kept = self._kept.get(key)
            track = self._track.get(key)
            held = self._held + (1 if track is not None and track.alias is not None else 0)  # our alias holds one too
            if kept is not None and kept.storage is not None and _use_count(kept.storage._cdata) > held:
                self.stats["held_by_caller"] += 1
                self._drop_tracks(key)  # the caller can still write it: nothing to vouch for next time
                return torch.empty_like(acts, memory_format=torch.contiguous_format), None  # still held by the caller
            storage = None
            vouch = False
            if kept is not None and kept.nbytes >= nbytes:
                ptr, kb, gbps, misses = kept.ptr, kept.nbytes, kept.gbps, kept.misses
                if kept.storage is not None:
                    # untouched through torch since a committed tracked launch wrote it?
                    clean = (track is not None and track.committed and track.alias is not None and track.version is not None
                             and _version_of(track.alias) == track.version)
                    if track is not None:
                        track.alias = None
                    n0 = self._alloc_count(acts.device)
                    # the last reference: the caching allocator owns the block, with the caller's streams
                    self._kept[key] = _Kept(None, kb, gbps, ptr, misses)
                    kept = None
                    if self._on_release:
                        self._on_release(ptr)
                    buf = self._alloc(kb, acts.device)
                    n1 = self._alloc_count(acts.device)
                    # ... and nobody else was handed it in between: exactly our one allocation in the window
                    vouch = clean and n0 is not None and n1 is not None and n1 - n0 == 1
                else:
                    buf = self._alloc(kb, acts.device)  # (after a miss: the block sat in the allocator, not vouched)
                if buf.data_ptr() == ptr:
                    self.stats["reuse_hits"] += 1
                    storage = buf.untyped_storage()
                    self._kept[key] = _Kept(storage, kb, gbps)
                else:
                    # still in use on another stream (or another stream's pool): hand the other block out plainly
                    self.stats["reuse_misses"] += 1
                    self._drop_tracks(key)
                    storage = buf.untyped_storage()
                    if misses + 1 >= 2:
                        del self._kept[key]  # the fast block is gone for good: choose afresh next time
                    else:
                        self._kept[key] = _Kept(None, kb, gbps, ptr, misses + 1)
                    self.stats["handed_out"] += 1
                    out = torch.empty(0, dtype=acts.dtype, device=acts.device)
                    return out.set_(storage, 0, acts.shape, _contiguous_strides(acts.shape)), None
            else:
                self._drop_tracks(key)
                track = None
                if kept is not None:
                    del self._kept[key]
                    kept = None  # the old block goes back to the caching allocator before the new one is chosen
                kept = self._kept[key] = self._choose(nbytes, acts.device)
                storage = kept.storage
            self.stats["handed_out"] += 1
            out = torch.empty(0, dtype=acts.dtype, device=acts.device)
            out.set_(storage, 0, acts.shape, _contiguous_strides(acts.shape))
            return out, self._ticket(key, out, row_bytes, self._kept[key].nbytes, vouch)

    def _choose(self, nbytes: int, dev: torch.device) -> _Kept:
        cands: List[Tuple[float, torch.Tensor]] = []
        while True:
            buf = self._alloc(nbytes, dev)
            cands.append((self._probe(buf), buf))
            best = max(c[0] for c in cands)
            if best >= self.fast_gbps or len(cands) >= self.max_candidates:
                break
            if self._free(dev) < FREE_FACTOR * nbytes:
                break
        rate, buf = max(cands, key=lambda c: c[0])
        self.log.append({"bytes": nbytes, "candidates_gbps": [round(c[0], 1) for c in cands],
                         "kept_gbps": round(rate, 1)})
        kept = _Kept(buf.untyped_storage(), nbytes, rate)
        if len(cands) > 1:
            slower = [c[1].data_ptr() for c in cands if c[1] is not buf]
            del buf
            cands.clear()  # the slower candidate is unused now: back to the driver, not left cached beside ours
            for q in slower:
                if self._on_release:
                    self._on_release(q)
            self._release_unused()
        return kept

    def release(self) -> None:
        with self._lock:
            self._kept.clear()
            self._drop_tracks()


def _capturing(acts: torch.Tensor) -> bool:
    """Inside HIP-graph capture the probe cannot synchronise: the graph's own pool serves the gradient."""
    return acts.is_cuda and torch.cuda.is_current_stream_capturing()


def _contiguous_strides(shape) -> Tuple[int, ...]:
    st, acc = [], 1
    for d in reversed(tuple(shape)):
        st.append(acc)
        acc *= max(int(d), 1)
    return tuple(reversed(st))


ARENA = GradsArena()


def grads_like(acts: torch.Tensor) -> torch.Tensor:
    return ARENA.like(acts) if enabled() else torch.empty_like(acts, memory_format=torch.contiguous_format)


def grads_tracked(acts: torch.Tensor, row_elems: Optional[int] = None) -> Tuple[torch.Tensor, Optional[Ticket]]:
    """grads_like() with the row state of the kept block (GradsArena.like_tracked); no ticket: the untracked entry."""
    if enabled():
        return ARENA.like_tracked(acts, row_elems)
    return torch.empty_like(acts, memory_format=torch.contiguous_format), None


def forget() -> None:
    """Call after writing a gradient this module handed out through `.data` or a raw pointer (see the docstring)."""
    ARENA.forget()


def release() -> None:
    """Drop the kept gradient buffers (they return to the caching allocator)."""
    ARENA.release()
