"""Multi-GPU sharding of the bounce kernel: one process per GPU, FoV x wavelength blocks.

Rays are independent and every ray's random stream is keyed by its GLOBAL index
(RNG seed ``0x9E3779B9 * (gid + 1)``, MAIN:158; zero-state fix-up, GRTF:28-29), so any set
of whole FoV x wavelength blocks (layout ``gid = ((ii * NY + jj) * L + l) * R + r``,
MAIN:82-115) can be traced on any GPU and gives bit-identical results, provided each local
ray knows its global id (``GidMap``).

Assignment.  Ray lifetimes differ by FoV and wavelength, so contiguous block ranges load the
ranks unevenly (the same effect measured across the dies of one GPU).  The
default assignment is therefore *interleaved*: block ``b = fov * L + k`` goes to rank
``(fov + k) mod N`` (``rank_blocks``) -- every N-th FoV, with the wavelength rotating, so each rank
gets a representative mix of FoVs and wavelengths whatever N and L are; ``contiguous`` remains
available.

Replicas (weak scaling).  ``replica_shard`` gives rank r the WHOLE batch again as replica r: the
same FoV x wavelength blocks and ray columns, with global ids ``r * N + i`` (N rays per replica),
so its random streams are its own.  N ranks then trace the reference's kernel over the batch's
columns tiled N times (RNG seeded by global index, MAIN:158) -- per-GPU work fixed as N grows, the
shape bench.py measures at N > 1 -- and every rank writes every slab, so the collective is the
sum-reduce of the grid (the north star's single RCCL reduce of the eyebox over xGMI).

Collective.  Each rank writes only the eyebox slabs ``EB[l, n, m]`` of its own blocks, plus --
through the compiled-numba flat-offset aliasing of an out-coupling exactly on the eyebox edge
(GRTF:154-165) -- the first ``SPILL`` floats of the slab after one of its own.
``EyeboxGather`` gathers exactly those bytes to rank 0 (each rank sends ``nb x (9600 + SPILL)`` floats,
1/N of the grid, over its own xGMI link) and rank 0 assembles the grid; ``reduce_eyebox`` is the plain
sum-reduce of the whole grid (50.8 MB at 21x21).  Eyebox values are integer counts, so both reproduce the
single-GPU grid exactly.  That is the only collective on the path.  A job that wants only the efficiencies
and the evaluation moves no slabs at all: ``EyeboxReduce`` sum-reduces each rank's per-slab window sums (57
float64 per slab), again exactly.  All three take their slab indices from one ``SlabPlan``.

The tracer is pluggable (``trace_fn(rays, rng, eb, gid, num_iter)``, ``gid`` a ``GidMap``) so the
same sharding / stepping / collection code runs with the HIP kernel in production (``bench.py``,
the reference-flow driver) and with the CPU oracle in the multi-process CPU tests.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

from ._lib import STAT, check, load

MAX_TRACES_PER_CALL = 255   # wgrt_launch_opts.num_iter
EB_SLAB = 80 * 120          # one (wavelength, FoV) slab of matrix_EB (MAIN:37)
SPILL = 121                 # floats of the next slab an edge out-coupling can alias into (ix <= 120 at iy 80)


def block_range(n_blocks: int, world: int, rank: int) -> tuple[int, int]:
    """Contiguous block range of ``rank`` (sizes differ by at most one block)."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError(f"bad rank {rank} / world {world}")
    return rank * n_blocks // world, (rank + 1) * n_blocks // world


def rank_blocks(n_blocks: int, world: int, rank: int, assign: str = "interleaved", n_lambda: int = 1) -> np.ndarray:
    """Global block ids of ``rank`` (ascending): ``interleaved`` -- block ``fov * n_lambda + k`` to
    rank ``(fov + k) % world`` -- or ``contiguous`` (block_range)."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError(f"bad rank {rank} / world {world}")
    if assign == "interleaved":
        b = np.arange(n_blocks, dtype=np.int64)
        return b[(b // n_lambda + b % n_lambda) % world == rank]
    if assign == "contiguous":
        lo, hi = block_range(n_blocks, world, rank)
        return np.arange(lo, hi, dtype=np.int64)
    raise ValueError(f"unknown assignment {assign!r}")


@dataclass
class GidMap:
    """Global id of local ray i: ``block_gid[i // rays_per_block] + i % rays_per_block``."""
    block_gid: np.ndarray
    rays_per_block: int

    @property
    def offset(self) -> int | None:
        """The single ``gid_offset`` when the blocks are consecutive, else None."""
        b, R = self.block_gid, self.rays_per_block
        if len(b) == 0:
            return 0
        return int(b[0]) if np.array_equal(b, b[0] + R * np.arange(len(b))) else None

    def device_blocks(self, device):
        """``block_gid`` as an int64 tensor on ``device`` (wgrt_launch_opts.gid_blocks), uploaded on first
        use and cached on this map."""
        import torch
        cache = self.__dict__.setdefault("_dev", {})
        key = str(device)
        if key not in cache:
            cache[key] = torch.as_tensor(self.block_gid, dtype=torch.int64, device=device)
        return cache[key]

    def runs(self):
        """Consecutive stretches: ``(local_ray_lo, local_ray_hi, global_gid_lo)``."""
        b, R = self.block_gid, self.rays_per_block
        i = 0
        while i < len(b):
            j = i + 1
            while j < len(b) and b[j] == b[j - 1] + R:
                j += 1
            yield i * R, j * R, int(b[i])
            i = j


@dataclass
class Shard:
    rank: int
    world: int
    blocks: np.ndarray            # global block ids, ascending
    rays_per_block: int
    assign: str = "interleaved"
    gid_base: int = 0             # global id of the first ray of block 0 (replica r: r * rays of the batch)
    _gid: GidMap | None = field(default=None, repr=False)

    @property
    def n_rays(self) -> int:
        return len(self.blocks) * self.rays_per_block

    @property
    def gid(self) -> GidMap:
        if self._gid is None:
            self._gid = GidMap(self.gid_base + self.blocks * self.rays_per_block, self.rays_per_block)
        return self._gid

    @property
    def gid_offset(self) -> int | None:
        return self.gid.offset


def make_shard(num_fov_x: int, num_fov_y: int, n_lambda: int, rays_per_fov: int, world: int,
               rank: int, assign: str = "interleaved") -> Shard:
    return Shard(rank, world, rank_blocks(num_fov_x * num_fov_y * n_lambda, world, rank, assign, n_lambda),
                 rays_per_fov, assign)


def replica_shard(num_fov_x: int, num_fov_y: int, n_lambda: int, rays_per_fov: int, world: int,
                  rank: int) -> Shard:
    """Replica ``rank`` of the whole batch (weak scaling): every block, global ids offset by
    ``rank`` times the batch's ray count."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError(f"bad rank {rank} / world {world}")
    nb = num_fov_x * num_fov_y * n_lambda
    return Shard(rank, world, np.arange(nb, dtype=np.int64), rays_per_fov, "replica",
                 gid_base=rank * nb * rays_per_fov)


def seeds_like(rng, gid: "GidMap"):
    """RNG seeds ``0x9E3779B9 * (gid + 1)`` (MAIN:158) of a shard's rays, written into ``rng``
    (a torch int32 view of the uint32 states, or a numpy uint32 array)."""
    R = gid.rays_per_block
    if hasattr(rng, "is_cuda"):
        import torch
        b = torch.as_tensor(gid.block_gid, dtype=torch.int64, device=rng.device)
        g = (b[:, None] + torch.arange(R, dtype=torch.int64, device=rng.device)[None, :]).reshape(-1)
        v = ((g + 1) * 0x9E3779B9) & 0xFFFFFFFF
        rng.copy_(torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32))
        return rng
    g = (np.asarray(gid.block_gid, dtype=np.uint64)[:, None] + np.arange(R, dtype=np.uint64)[None, :]).reshape(-1)
    rng[:] = ((g + np.uint64(1)) * np.uint64(0x9E3779B9) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return rng


def slab_ids(blocks, num_fov_x: int, num_fov_y: int, lambdas) -> np.ndarray:
    """Flat slab index ``(lambda * NY + n) * NX + m`` of matrix_EB for each global block
    ``((m * NY + n) * L + k) * R`` (MAIN:82-115; lambda = lambdas[k])."""
    b = np.asarray(blocks, dtype=np.int64)
    L = len(lambdas)
    fov, k = np.divmod(b, L)
    m, n = np.divmod(fov, num_fov_y)
    lam = np.asarray(lambdas, dtype=np.int64)[k]
    return (lam * num_fov_y + n) * num_fov_x + m


def split_calls(steps: int, per_call: int = 1) -> list[int]:
    """``steps`` chained traces as calls of at most ``per_call`` traces each (0: as few calls as
    possible), each call at most ``MAX_TRACES_PER_CALL``."""
    if steps < 0:
        raise ValueError("steps must be >= 0")
    f = min(MAX_TRACES_PER_CALL, steps if per_call <= 0 else per_call) or 1
    out = []
    while steps > 0:
        out.append(min(f, steps))
        steps -= out[-1]
    return out


def run_steps(trace_fn, rays, rng, eb, gid: GidMap, steps: int, per_call: int = 1, hook=None) -> list[int]:
    """The reference's loop of chained launches (MAIN:169-177) over one shard: ``steps`` traces
    of every ray, each starting from the RNG states the previous one left, issued as calls of
    at most ``per_call`` traces (``trace_fn(..., num_iter=k)``; a fused call gives the results
    of k separate ones).  ``eb`` is handed to ``trace_fn`` as it is: None for a tracer that carries the
    window-table sink alone (``hip_tracer(windows=...)``).  ``hook(j, "start" | "end")`` brackets call j (HIP events in bench.py).
    Separate launches (``per_call == 1``, more than one step, no hook) of a tracer that offers ``chain`` are issued
    through it.  ``hip_tracer``'s chain gathers (``engine.TraceChain(gather=True)``): this loop calls its steps back
    to back and reads nothing in between, so the steps called while the GPU is still busy go out as fused launches --
    the same results, fewer launches than traces.
    Returns the traces per call."""
    calls = split_calls(steps, per_call)
    chain = getattr(trace_fn, "chain", None)
    if chain is not None and per_call == 1 and steps > 1 and hook is None:
        # separate traces all the same, issued through the tracer's chain (hip_tracer: a gathering one).  With a hook
        # the calls stay plain launches: it brackets each one on the stream
        with chain(rays, rng, eb, gid) as ch:
            for _ in calls:
                ch.step()
        return calls
    for j, k in enumerate(calls):
        if hook is not None:
            hook(j, "start")
        trace_fn(rays, rng, eb, gid, k)
        if hook is not None:
            hook(j, "end")
    return calls


def _world(group):
    import torch.distributed as dist
    return dist.get_world_size(group) if dist.is_initialized() else 1


def _operands(group, *tensors, scratch: bool = False):
    """What a collective is handed for ``tensors``: the tensors themselves, except under gloo (the CPU tests, the
    one-GPU rehearsals), which moves host tensors only and whose reduce leaves partial sums in the other ranks'
    operands: there a device tensor goes as a host copy and a host tensor the collective may overwrite
    (``scratch``) as a clone.  The caller copies a result back where it was handed a copy."""
    import torch.distributed as dist
    if dist.get_backend(group) != "gloo":
        return tensors
    return tuple(t.cpu() if t.is_cuda else t.clone() if scratch else t for t in tensors)


def reduce_eyebox(eb, group=None, dst: int = 0):
    """Sum-reduce the eyebox grid (or ``EyeboxReduce``'s table) to rank ``dst``, in place there; every other rank's
    tensor stays as it was.  Exact: integer counts, in float32 below 2**24."""
    import torch.distributed as dist
    if _world(group) > 1:
        at_dst = dist.get_rank(group) == dst
        buf, = _operands(group, eb, scratch=not at_dst)
        dist.reduce(buf, dst=dst, op=dist.ReduceOp.SUM, group=group)
        if at_dst and buf is not eb:
            eb.copy_(buf)
    return eb


class SlabPlan:
    """One block assignment's index sets (``all_blocks[r]``: global block ids of rank r), computed once in numpy.

    Two per rank r: ``slabs[r]``, the eyebox slab of each of its blocks in block order (not ascending), and
    ``spill[r]``, whether that slab's spill must travel -- it lands in slab s + 1 and moves unless s + 1 is the
    rank's own slab (then it is in that slab's copy already) or past the grid (dropped, as the kernel's guard
    drops it).  The rest follows from them: ``nxt`` (where a row's spill is read, clamped to the grid),
    ``spill_rows`` / ``spill_dst`` (the payload rows with a spill, the slabs they add to), ``rows`` (every slab
    the rank can have written: its own, then the spill targets that are not, no slab twice), ``unowned`` (slabs
    of no rank), and ``wgrt_eyebox_assemble``'s flat row maps: payload row j of rank r goes to slab
    ``dst_rows[r * nb + j]`` and its spill adds to ``spill_dst_rows[r * nb + j]``, -1 for none."""

    def __init__(self, all_blocks, num_fov_x: int, num_fov_y: int, lambdas, n_lambda_scene: int):
        n = self.n_slabs = n_lambda_scene * num_fov_y * num_fov_x
        self.world = len(all_blocks)
        self.slabs = [slab_ids(b, num_fov_x, num_fov_y, lambdas) for b in all_blocks]
        self.spill = [~np.isin(s + 1, s) & (s + 1 < n) for s in self.slabs]
        self.counts = [len(s) for s in self.slabs]
        self.nb = max(self.counts)
        self.has_spill = [bool(m.any()) for m in self.spill]
        self.nxt = [np.minimum(s + 1, n - 1) for s in self.slabs]
        self.spill_rows = [np.nonzero(m)[0] for m in self.spill]
        self.spill_dst = [s[m] + 1 for s, m in zip(self.slabs, self.spill)]
        self.rows = [np.concatenate([s, d]) for s, d in zip(self.slabs, self.spill_dst)]
        self.unowned = np.setdiff1d(np.arange(n), np.concatenate(self.slabs))
        dst = np.full((2, self.world, self.nb), -1, dtype=np.int64)
        for r, s in enumerate(self.slabs):
            dst[0, r, :len(s)] = s
            dst[1, r, self.spill_rows[r]] = self.spill_dst[r]
        self.dst_rows, self.spill_dst_rows = dst[0].reshape(-1), dst[1].reshape(-1)
        self.tensors = {}

    def on(self, device):
        """The plan as tensors on ``device`` (int64; ``spill`` as the float32 factor the pack multiplies by),
        uploaded on first use and kept in ``tensors``: the indices live where the grid they index lives."""
        import torch
        key = str(device)
        if key not in self.tensors:
            t = lambda a, dt=torch.int64: torch.as_tensor(a, dtype=dt, device=device)
            per_rank = ("slabs", "nxt", "spill_rows", "spill_dst", "rows")
            self.tensors[key] = SimpleNamespace(
                spill=[t(m, torch.float32) for m in self.spill], unowned=t(self.unowned), dst_rows=t(self.dst_rows),
                spill_dst_rows=t(self.spill_dst_rows), **{k: [t(a) for a in getattr(self, k)] for k in per_rank})
        return self.tensors[key]


class EyeboxGather:
    """Gather of each rank's own eyebox slabs (+ their spill) to rank 0, and the assembly there.

    Every rank knows the whole assignment (``SlabPlan``), so the message sizes and placements need no exchange.
    A rank's payload is one flat buffer, ``[nb x 9600 slab floats | nb x SPILL spill floats, padded to 4]``
    (include/wgrt.h wgrt_eyebox_*), padded to the largest shard (the collective needs equal sizes).  The send
    buffer and rank 0's receive buffer are allocated once (first call per device and dtype) and reused, and the
    plan's tensors are uploaded once per device (``device=``: up front), so a call makes no host round trip before
    the collective.  On a HIP device a contiguous float32 grid is packed and assembled by the library's row-copy
    kernels (``wgrt_eyebox_pack`` / ``wgrt_eyebox_assemble``: one launch each, 16-B loads and stores, each owned
    slab written once from the rank that traced it); any other tensor takes the same steps as torch gathers and
    scatters on its own device.  Slabs no rank owns are zeroed, spills added last."""

    def __init__(self, all_blocks, num_fov_x: int, num_fov_y: int, lambdas, n_lambda_scene: int, device=None):
        p = self.plan = SlabPlan(all_blocks, num_fov_x, num_fov_y, lambdas, n_lambda_scene)
        self.n_slabs, self.world, self.nb, self.counts, self.has_spill = p.n_slabs, p.world, p.nb, p.counts, p.has_spill
        self.payload_len = self.nb * EB_SLAB + (self.nb * SPILL + 3) // 4 * 4
        self._bufs = {}
        if device is not None:
            p.on(device)

    def buffers(self, device, dtype, dst: bool):
        """(send, recv): the payload buffer and, on the gathering rank, the [world, payload] receive
        buffer (None elsewhere); allocated on first use, zeroed once (padding rows stay zero)."""
        import torch
        key = (str(device), dtype, dst)
        if key not in self._bufs:
            send = torch.zeros(self.payload_len, dtype=dtype, device=device)
            recv = torch.zeros((self.world, self.payload_len), dtype=dtype, device=device) if dst else None
            self._bufs[key] = (send, recv)
        return self._bufs[key]

    def _views(self, buf):
        nb = self.nb
        return buf[:nb * EB_SLAB].view(nb, EB_SLAB), buf[nb * EB_SLAB:nb * EB_SLAB + nb * SPILL].view(nb, SPILL)

    @staticmethod
    def _hip(t) -> bool:
        return t.is_cuda and t.dtype.is_floating_point and t.element_size() == 4 and t.is_contiguous()

    @staticmethod
    def _kernel(name: str, eb, *args) -> None:
        """The library's row-copy kernel ``name`` on grid ``eb``, on torch's current stream of its device."""
        from .engine import _stream_handle
        check(getattr(load(), name)(eb.data_ptr(), *args, _stream_handle(eb.device)), name)

    def pack(self, eb, rank: int, out=None):
        """Rank ``rank``'s payload, into ``out`` (the collective passes its reused send buffer) or a new
        zeroed buffer.  ``eb`` may have any layout."""
        import torch
        buf = out if out is not None else torch.zeros(self.payload_len, dtype=eb.dtype, device=eb.device)
        n = self.counts[rank]
        ix = self.plan.on(eb.device)
        if self._hip(eb):
            if buf.device != eb.device or not buf.is_contiguous() or buf.numel() < self.payload_len:
                raise ValueError("EyeboxGather.pack: out must be a contiguous payload buffer on the grid's device")
            self._kernel("wgrt_eyebox_pack", eb, self.n_slabs, ix.slabs[rank].data_ptr(), ix.nxt[rank].data_ptr(),
                         ix.spill[rank].data_ptr(), n, self.nb, buf.data_ptr())
            return buf
        flat = eb.reshape(self.n_slabs, EB_SLAB)
        main, spill = self._views(buf)
        torch.index_select(flat, 0, ix.slabs[rank], out=main[:n])
        if self.has_spill[rank]:
            torch.index_select(flat[:, :SPILL], 0, ix.nxt[rank], out=spill[:n])
            spill[:n].mul_(ix.spill[rank].to(eb.dtype)[:, None])
        return buf

    def assemble(self, eb, parts) -> None:
        """Rank 0: rebuild the whole grid in ``eb`` (contiguous: it is written in place) from every rank's
        payload (``parts[r]``: rank r's flat payload; ``parts`` may be the [world, payload] receive buffer)."""
        import torch
        if not eb.is_contiguous():
            raise ValueError("EyeboxGather.assemble: the grid must be contiguous (it is written in place)")
        flat = eb.view(self.n_slabs, EB_SLAB)
        ix = self.plan.on(eb.device)
        if len(self.plan.unowned):
            flat.index_fill_(0, ix.unowned, 0)
        if self._hip(eb):
            recv = parts if hasattr(parts, "shape") else torch.stack(list(parts))
            recv = recv if recv.device == eb.device and recv.is_contiguous() else recv.to(eb.device).contiguous()
            self._kernel("wgrt_eyebox_assemble", eb, self.n_slabs, recv.data_ptr(), self.world, self.nb,
                         ix.dst_rows.data_ptr(), ix.spill_dst_rows.data_ptr())
            return
        views = [self._views(parts[r]) for r in range(self.world)]
        for r, (main, _) in enumerate(views):
            flat.index_copy_(0, ix.slabs[r], main[:self.counts[r]])
        for r, (_, spill) in enumerate(views):   # an empty index set adds nothing
            flat[:, :SPILL].index_add_(0, ix.spill_dst[r], spill.index_select(0, ix.spill_rows[r]))

    def __call__(self, eb, group=None, dst: int = 0):
        import torch.distributed as dist
        if _world(group) <= 1:
            return eb
        rank = dist.get_rank(group)
        send, recv = self.buffers(eb.device, eb.dtype, rank == dst)
        payload, = _operands(group, self.pack(eb, rank, out=send))
        rows = recv.unbind(0) if rank == dst else ()
        parts = _operands(group, *rows)
        dist.gather(payload, gather_list=list(parts) if rank == dst else None, dst=dst, group=group)
        if rank == dst:
            for row, part in zip(rows, parts):
                if part is not row:
                    row.copy_(part)
            self.assemble(eb, recv)
        return eb


class EyeboxReduce:
    """The evaluation-only collective: each rank reduces its own part of the grid to per-slab window sums
    (``AR_system_evaluation_functions.eyebox_window_sums``: the slab total and the 7 x 8 pupil sums, 57 float64 per
    slab) and ONE sum-reduce of the ``[n_slabs, W]`` table brings them to rank 0, instead of whole 38.4 KB slabs.

    A rank reduces only the slabs it can have written (``SlabPlan.rows``: its own blocks' and, for the H6 top-edge
    spill, the slab after each), into a zeroed table.  Window sums are linear in the grid and the grid holds
    integer counts, so every entry is an integer, exact in float64 whatever the order of the additions: rank 0's
    table equals the window sums of the assembled grid bit for bit, spills into slabs no rank owns included.  A
    device grid is reduced by the HIP kernel; host tensors by the numpy statement of the same formula."""

    def __init__(self, all_blocks, num_fov_x: int, num_fov_y: int, lambdas, n_lambda_scene: int, mask=None,
                 step_y: int = 8, step_x: int = 12):
        self.plan = SlabPlan(all_blocks, num_fov_x, num_fov_y, lambdas, n_lambda_scene)
        self.n_slabs, self.world = self.plan.n_slabs, self.plan.world
        self.rows = self.plan.on("cpu").rows
        self.mask, self.step_y, self.step_x = mask, step_y, step_x

    def local(self, eb, rank: int):
        """Rank ``rank``'s contribution: its rows' window sums scattered into a zeroed ``[n_slabs, W]`` float64
        tensor on the grid's device."""
        import torch

        from .AR_system_evaluation_functions import eyebox_window_sums
        rows = self.plan.on(eb.device).rows[rank]
        part = torch.as_tensor(eyebox_window_sums(eb, rows, self.mask, self.step_y, self.step_x))
        full = torch.zeros((self.n_slabs, part.shape[1]), dtype=torch.float64, device=eb.device)
        return full.index_copy_(0, rows, part)

    def __call__(self, eb, group=None, dst: int = 0):
        """Rank ``dst``: the ``[n_slabs, W]`` window sums of the whole job's grid (elsewhere: this rank's own part)."""
        import torch.distributed as dist
        return reduce_eyebox(self.local(eb, dist.get_rank(group) if _world(group) > 1 else 0), group, dst)


def trace_job(shard: Shard, build_rays_fn, trace_fn, new_eb, num_iter: int = 4, per_call: int = 1, group=None,
              collect=None):
    """Run the reference's job (``num_iter`` chained launches, MAIN:169-177) on this rank's
    shard and collect the eyebox grid on rank 0.

    build_rays_fn(shard) -> (rays, rng) for the shard (rng seeded with the global ids);
    trace_fn(rays, rng, eb, gid, num_iter) performs num_iter chained traces in place;
    new_eb() -> zeroed eyebox grid (numpy array or torch tensor); collect(eb, group) ->
    the collective (default ``reduce_eyebox``; an ``EyeboxGather`` moves 1/N of the bytes).
    Returns (eb, rng): eb holds the full-job grid on rank 0 (this rank's partial elsewhere).
    """
    rays, rng = build_rays_fn(shard)
    eb = new_eb()
    if shard.n_rays:
        run_steps(trace_fn, rays, rng, eb, shard.gid, num_iter, per_call)
    return (collect or reduce_eyebox)(eb, group), rng


def timed_run(trace_fn, rays, rng, eb, gid: GidMap, steps: int, per_call: int, stats, sync=None, hook=None,
              group=None, collect=None):
    """bench.py's timed region on one rank: barrier + ``sync()``, ``steps`` chained traces of the
    shard (``run_steps``), the eyebox collective to rank 0 (``collect``, default the reduce),
    ``sync()`` + barrier.  ``stats[STAT.bounces]`` (the device bounce counter, zeroed here) is what the
    tracer adds to.  Returns ``(elapsed, bounces, bounces_local)``: the wall time MAX over ranks,
    the bounce total SUM over ranks, this rank's own bounces.  The two small all-reduces run on
    ``stats``'s device (RCCL on the GPU box, gloo in the CPU tests)."""
    import time

    import torch
    import torch.distributed as dist
    multi = _world(group) > 1
    sync = sync or (lambda: None)
    stats.zero_()
    if multi:
        dist.barrier(group)
    sync()
    t0 = time.perf_counter()
    if steps and (rng.numel() if hasattr(rng, "numel") else len(rng)):
        run_steps(trace_fn, rays, rng, eb, gid, steps, per_call, hook)
    (collect or reduce_eyebox)(eb, group)
    sync()
    if multi:
        dist.barrier(group)
    elapsed = time.perf_counter() - t0
    local = int(stats[STAT.bounces].item())
    t = torch.tensor([elapsed], dtype=torch.float64, device=stats.device)
    b = torch.tensor([local], dtype=torch.int64, device=stats.device)
    if multi:
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        dist.all_reduce(b, op=dist.ReduceOp.SUM, group=group)
    return float(t.item()), int(b.item()), local


def hip_tracer(scene, variant: int = 0, stats=None, windows=None, fate=None, replicas: int = 0,
               expected: bool = False, footprint=None, hits=None, paths=None, visits=None, stokes=None):
    """trace_fn for ``run_steps`` / ``trace_job`` using the HIP kernel (torch device tensors); ``stats``
    (int64[STATS_LEN] device tensor) is added to by every call.  A shard of several block ranges passes its global
    ids as ``gid_blocks``, uploaded once per map and device and kept on the map (``GidMap.device_blocks``).

    ``windows=(plan, table)``: every call also counts its out-couplings into the pupil-window table
    (``engine.trace_fullcolor(windows=...)``), and ``eb`` may be None -- a grid-free job.  Every rank's table is
    the full ``[n_slabs, W]`` with its top-edge spills already in the slabs they alias into, so the collective
    of such a job is ``reduce_eyebox(table)``, one sum-reduce: no slab list, no scatter.

    ``fn.chain(rays, rng, eb, gid)`` returns an ``engine.TraceChain`` over the same arguments: a context whose
    ``step()`` is one such call with ``num_iter = 1``.  It is a gathering chain (``gather=True``): what uses it
    (``run_steps``) calls the steps back to back and touches nothing before the chain ends.

    ``fate``: a uint8 device tensor every call stores the rays' fate codes in (``engine.trace_fullcolor(fate=...)``:
    single launches only, so ``num_iter`` must stay 1); such a tracer offers no ``chain`` (a chain takes no fates),
    so ``run_steps`` issues its launches plain, and a ``hook`` can census the buffer after each.

    ``replicas``: ``B``, with ``windows=(plan, table)`` and ``table`` the ``[B, n_slabs, W]`` replica tables
    (``engine.trace_fullcolor(replicas=...)``): single launches only again, and no ``chain``.  A ray's replica is its
    global id's, so the ranks' replica tables add: the collective is still ``reduce_eyebox(table)``.

    ``expected``: every call scores the expected-value estimator into the table instead
    (``engine.trace_fullcolor(expected=True)``; ``eb`` must be None): single launches only and no ``chain`` again.
    The sums are exact multiples of 2^-32, so the ranks' tables add exactly, as the counts do.

    ``footprint``: ``(fp, map)``, an ``engine.FootprintPlan`` and its int64 map: every call also counts its draws into
    the plate map (``engine.trace_fullcolor(footprint=...)``): single launches only and no ``chain`` again.  The
    counts are integers, so the ranks' maps add: ``reduce_eyebox(map)``.

    ``hits``: an ``engine.HitList``: every call also appends its out-couplings to the list
    (``engine.trace_fullcolor(hits=...)``), tagged with the number of calls made before it (the iteration, for the
    single launches this takes): single launches only and no ``chain`` again.  The records' ids are global, so the
    ranks' lists concatenate.

    ``paths``: a record with ``list`` (an ``engine.PathList``), ``classes`` (fate class names or codes, or None for every
    ray), ``selected`` (int64 ``[num_lmd]`` device tensor, added to: the rays recorded per wavelength) and, for a class
    selection, ``fate`` (uint8 per ray), ``windows`` (a scratch plan and table) and optionally ``bounces`` (int32 per ray:
    the first pass then stores its per-ray bounces there, and the list is grown before the paths launch to hold
    ``bounces + 1`` records of every selected ray, so that it cannot overflow): every call records the draws of the
    selected rays in the list (``engine.trace_fullcolor(paths=..., select=...)``), tagged like ``hits``.  For a class
    selection the call first runs a fate launch with no grid on a clone of the RNG states into the scratch table,
    builds the mask from its fates (``engine.select_by_fate``), and then runs the paths launch from the original
    states.  Single launches only and no ``chain`` again; the ids are global, so the ranks' lists concatenate.

    ``visits``: a record with ``plan`` (the job's ``engine.WindowPlan``), ``fate`` (uint8 per ray), ``windows`` (a scratch
    plan and table), ``sens`` (float64 ``[C, n_slabs, W]``, added to; None: no sensitivities are wanted) and, for a what-if, ``scales`` (``{channel: s}``),
    ``table`` (float64 ``[n_slabs, W]``, added to) and ``sums`` (float64 ``[2, num_lmd]``, added to: the weights' sum and
    sum of squares) and, for a design ensemble, ``ensemble`` (a record with ``scales``, K designs as
    ``VisitTable.reweight_many`` takes them, ``tables`` float64 ``[K, n_slabs, W]`` and ``sums`` int64
    ``[K, 2, num_lmd]``, both added to): every call first runs a fate launch with no grid on a clone of the RNG states into the scratch table,
    gives the rays of the ``eyebox`` class the rows 0, 1, ... (an exclusive cumsum of the mask), runs the visits launch
    from the original states (``engine.trace_fullcolor(visits=...)``) and reduces its rows into ``sens`` (and ``table``).
    Single launches only and no ``chain`` again; the tables are sums over rays, so the ranks' tables add.

    ``stokes``: an ``engine.StokesTable`` of the job's plan (needs ``windows``): every call also adds the Stokes quanta of
    the out-couplings its window table counts to the int64 tables (``engine.trace_fullcolor(stokes=...)``): single
    launches only and no ``chain`` again.  Integer sums: the ranks' tables add exactly, ``reduce_eyebox(stokes.raw())``."""
    from .engine import TraceChain, VisitTable, select_by_fate, trace_fullcolor
    calls = [0]

    def visits_for(rays, rng, gid):
        """The visits launch's table and slots: the delivered rays, one row each."""
        import torch
        trace_fullcolor(scene, rays, rng.clone(), None, variant=variant, windows=visits.windows, fate=visits.fate,
                        **ids_of(rng, gid))
        mask = select_by_fate(visits.fate, "eyebox").to(torch.int32)
        first = torch.cumsum(mask, 0, dtype=torch.int32) - mask          # exclusive
        slot = torch.where(mask != 0, first, torch.full_like(first, -1))
        return VisitTable(scene, int(mask.sum().item())), slot           # (synchronises)

    def reduce_visits(vt):
        if visits.sens is not None:
            vt.sensitivity(visits.plan, out=visits.sens)
        if getattr(visits, "scales", None) is not None:
            vt.reweight(visits.plan, visits.scales, out=visits.table)
            visits.sums += vt.weight_sums(visits.scales)
        ens = getattr(visits, "ensemble", None)
        if ens is not None:
            vt.reweight_many(visits.plan, ens.scales, out=ens.tables, sums=ens.sums)

    def select_for(rays, rng, gid):
        """The paths launch's mask (None: every ray), the rays it names counted per wavelength."""
        import torch
        lmd = rays["lmd_num"].long()
        if paths.classes is None:
            paths.selected += torch.bincount(lmd, minlength=paths.selected.numel())
            return None
        bounces = getattr(paths, "bounces", None)
        trace_fullcolor(scene, rays, rng.clone(), None, variant=variant, windows=paths.windows, fate=paths.fate,
                        per_ray_bounces=bounces, **ids_of(rng, gid))
        mask = select_by_fate(paths.fate, paths.classes)
        paths.selected += torch.bincount(lmd[mask != 0], minlength=paths.selected.numel())
        if bounces is not None:
            # the list sized from the first pass: a draw is made in a loop iteration, and every iteration counts a
            # bounce, so a selected ray leaves at most its bounces + 1 records (the end record).  Synchronises.
            need = int((bounces[mask != 0].long() + 1).sum().item())
            paths.list.reserve(paths.list.count() + need)
        return mask

    def ids_of(rng, gid: GidMap):
        off = gid.offset
        return dict(gid_offset=off) if off is not None else dict(gid_blocks=gid.device_blocks(rng.device),
                                                                 gid_block_rays=gid.rays_per_block)

    def fn(rays, rng, eb, gid: GidMap, num_iter=1):
        more = {} if paths is None else dict(paths=(paths.list, calls[0]), select=select_for(rays, rng, gid))
        if visits is not None:
            more = dict(visits=visits_for(rays, rng, gid))
        trace_fullcolor(scene, rays, rng, eb, stats=stats, variant=variant, num_iter=num_iter, windows=windows,
                        fate=fate, replicas=replicas, expected=expected, footprint=footprint,
                        hits=None if hits is None else (hits, calls[0]), stokes=stokes, **more, **ids_of(rng, gid))
        if visits is not None:
            reduce_visits(more["visits"][0])
        calls[0] += 1

    def chain(rays, rng, eb, gid: GidMap):
        """The same launches as a chain (``run_steps`` uses it for separate launches without a hook)."""
        # (a build of the library from before wgrt_chain_gather, tools/with_lib.py: the plain two-queue chain)
        from ._lib import load
        return TraceChain(scene, rays, rng, eb, stats=stats, variant=variant, windows=windows,
                          gather=hasattr(load(), "wgrt_chain_gather"), **ids_of(rng, gid))
    if fate is None and int(replicas or 0) < 2 and not expected and footprint is None and hits is None and paths is None \
            and visits is None and stokes is None:
        fn.chain = chain
    return fn


def hip_shard_builder(points, num_fov_x, num_fov_y, lambdas, rays_per_fov, device):
    """build_rays_fn for ``trace_job`` that lays the shard out on the device (``wgrt_rays_init``,
    MAIN:59-158 without host arrays): only the eight columns the kernel reads."""
    from .engine import init_rays

    def build(shard: Shard):
        rays, rng = init_rays(points, num_fov_x, num_fov_y, lambdas, rays_per_fov, block_list=shard.blocks,
                              device=device, all_columns=False)
        if shard.gid_base:   # a replica: the same columns, its own global ids
            seeds_like(rng, shard.gid)
        return rays, rng
    return build


def shard_rays_host(points, num_fov_x, num_fov_y, lambdas, rays_per_fov, blocks, gid_base: int = 0):
    """Host SoA columns + seeds of the global blocks ``blocks`` laid back to back (rays.build_rays
    restricted to each run of consecutive blocks); ``gid_base`` offsets the global ids (a replica
    shard)."""
    from .rays import build_rays, rng_seeds
    parts, seeds = [], []
    R = rays_per_fov
    for lo_r, hi_r, g in GidMap(np.asarray(blocks, dtype=np.int64) * R, R).runs():
        b0 = g // R
        nb = (hi_r - lo_r) // R
        parts.append(build_rays(points, num_fov_x, num_fov_y, lambdas, R, blocks=(b0, b0 + nb)))
        seeds.append(rng_seeds(nb * R, g))
    if not parts:
        empty = build_rays(points, num_fov_x, num_fov_y, lambdas, R, blocks=(0, 0))
        return empty, rng_seeds(0, 0)
    rays = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    seeds = np.concatenate(seeds)
    if gid_base:
        seeds_like(seeds, GidMap(gid_base + np.asarray(blocks, dtype=np.int64) * R, R))
    return rays, seeds


__all__ = ["block_range", "rank_blocks", "GidMap", "Shard", "make_shard", "replica_shard", "seeds_like", "slab_ids", "split_calls", "run_steps",
           "reduce_eyebox", "EyeboxGather", "EyeboxReduce", "trace_job", "timed_run", "hip_tracer", "hip_shard_builder",
           "shard_rays_host", "SlabPlan", "MAX_TRACES_PER_CALL", "EB_SLAB", "SPILL"]
