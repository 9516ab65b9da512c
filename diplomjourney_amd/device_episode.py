"""The device-resident MPC episode (mpc_episode_* C ABI) and the step
structures a chained episode can run: one class per structure, each owning
its launch, its flush and what its pending value means."""
import ctypes
import weakref

import torch

from . import native
from .abi import (CANDIDATE_BYTES, INTEGRATORS, IPC_HANDLE_BYTES, LOG_BYTES, MPC_LAYOUT_TILED,
                  MPC_MAX_OBSTACLES, MPC_MAX_POLYGONS, MPC_TILE, RESULT_BYTES, MpcEpisodeLog,
                  make_obstacles, make_polygons, polygon_is_convex, polygon_vertices)
from .distributed import gather_bytes, gather_into, gather_results, reduce_int, shard_range
from .episode_config import ChainError, reference_episode_config
from .streams import _check_overlap_stream


def _is_tiled(controls):
    return isinstance(controls, torch.Tensor)


def _stop(events):
    if events:
        events[1].record()


class _ChainForm:
    """One chained step structure.  launch(ep, ctl, pend, events) enqueues the
    rollout of the step over `ctl` with the completion of the step `pend`
    stands for (None: none is pending), records events[1] behind the launch
    and returns the new pending value; flush(ep, pend) completes the last
    step.  The pending value lives on the episode (ep._pending), the epoch that
    belongs to it in the form."""
    pends_controls = False   # pending is the previous step's controls (either layout)

    def close(self):
        pass


class _OneGpuChain(_ChainForm):
    """mpc_episode_chain_step (with circles: _chain_step_obstacles, with
    polygons: _chain_step_keepout) / mpc_episode_finalize."""
    pends_controls = True

    def launch(self, ep, ctl, pend, events):
        vp, bp, integ = ep._ptrs(ctl)
        ws, ws_prev = ep._ws
        args = (1, ep._next_epoch(), vp, bp, *ep._shard, integ, ws.data_ptr(),
                ws_prev.data_ptr(), ws.numel(), *ep._prev_ptrs(pend), ep.local.data_ptr(), None, 0)
        ep._entry("mpc_episode_chain_step", ep._head, *args, *ep._tail())
        _stop(events)
        return ctl

    def flush(self, ep, pend):
        vp, bp, integ = ep._ptrs(pend)
        ws = ep._ws[1]
        ep._C.mpc_episode_finalize(
            ep.state.data_ptr(), vp, bp, *ep._shard, integ, ws.data_ptr(), ws.numel(),
            ep.local.data_ptr(), ctypes.byref(ep.cfg), *ep._tail())


class _P2PChain(_ChainForm):
    """mpc_episode_p2p_step / _flush: one launch per step and no collective —
    block 0 posts this rank's candidate of step k-1 to every mailbox over
    xGMI, waits for the world's, selects and updates.  The previous controls
    pend with the epoch they were launched under."""
    pends_controls = True

    def __init__(self, mailbox):
        self.mailbox = mailbox
        self.prev_epoch = 0

    def launch(self, ep, ctl, pend, events):
        vp, bp, integ = ep._ptrs(ctl)
        ws, ws_prev = ep._ws
        epoch = ep._next_epoch()
        ep._C.mpc_episode_p2p_step(
            *ep._head, epoch, self.prev_epoch if pend is not None else 0, vp, bp,
            *ep._shard, integ, ws.data_ptr(), ws_prev.data_ptr(), ws.numel(),
            *ep._prev_ptrs(pend), ctypes.c_void_p(self.mailbox.ptr), ep.world,
            ep.winner.data_ptr(), *ep._tail())
        _stop(events)
        self.prev_epoch = epoch
        return ctl

    def flush(self, ep, pend):
        vp, bp, integ = ep._ptrs(pend)
        ws = ep._ws[1]
        ep._C.mpc_episode_p2p_flush(
            *ep._head, self.prev_epoch, vp, bp, *ep._shard, integ, ws.data_ptr(), ws.numel(),
            ctypes.c_void_p(self.mailbox.ptr), ep.world, ep.winner.data_ptr(), *ep._tail())


class _GatheredChain(_ChainForm):
    """mpc_episode_exchange_step, then ONE all_gather of the ranks' 536-B
    candidates; the next launch (or mpc_episode_exchange_flush) selects over
    them.  The gathered bytes pend."""

    def launch(self, ep, ctl, pend, events):
        vp, bp, _ = ep._ptrs(ctl)
        ws = ep._ws[0]
        ep._C.mpc_episode_exchange_step(
            *ep._head, ep._next_epoch(), vp, bp, *ep._shard, ep._integ, ws.data_ptr(),
            ws.numel(), pend.data_ptr() if pend is not None else None,
            ep.world if pend is not None else 0, ep.winner.data_ptr(), ep.cand.data_ptr(),
            *ep._tail())
        _stop(events)                    # the launch alone, not the collective after it
        return gather_bytes(ep.cand, ep.group)

    def flush(self, ep, pend):
        ep._C.mpc_episode_exchange_flush(*ep._head, ep._integ, pend.data_ptr(), ep.world,
                                         ep.winner.data_ptr(), *ep._tail())


class _OverlappedChain(_GatheredChain):
    """The same launch (mpc_episode_exchange_step2), but the all_gather of step
    k runs on a side stream beside launch k+1, whose block 0 waits for its
    device-side mark (mpc_episode_exchange_mark).  The gather buffer pends
    with the epoch its mark carries."""

    def __init__(self, world, device):
        self.gathered = torch.zeros(world * CANDIDATE_BYTES, dtype=torch.uint8, device=device)
        self.comm = torch.cuda.Stream(device=device)
        self.pend_epoch = 0

    def launch(self, ep, ctl, pend, events):
        _check_overlap_stream()
        vp, bp, _ = ep._ptrs(ctl)
        ws = ep._ws[0]
        epoch = ep._next_epoch()
        ep._C.mpc_episode_exchange_step2(
            *ep._head, epoch, self.pend_epoch if pend is not None else 0, vp, bp,
            *ep._shard, ep._integ, ws.data_ptr(), ws.numel(),
            self.gathered.data_ptr() if pend is not None else None,
            ep.world if pend is not None else 0, ep.winner.data_ptr(), ep.cand.data_ptr(),
            *ep._tail())
        _stop(events)
        self.comm.wait_stream(torch.cuda.current_stream())   # after this launch (its candidate)
        with torch.cuda.stream(self.comm):
            gather_into(self.gathered, ep.cand, ep.group)
            ep._C.mpc_episode_exchange_mark(ep.state.data_ptr(), epoch,
                                            ctypes.c_void_p(self.comm.cuda_stream))
        self.pend_epoch = epoch
        return self.gathered

    def flush(self, ep, pend):
        torch.cuda.current_stream().wait_stream(self.comm)   # the last collective, then its step
        super().flush(ep, pend)

    def close(self):
        self.comm.synchronize()
        torch.cuda.current_stream().synchronize()


class _Mailbox:
    """One rank's P2P mailbox (mpc_mailbox_*) and its mappings of the peers'
    (mpc_ipc_*).  alloc, connect and self_test are the stages of the setup."""

    def __init__(self, device, rank, world):
        self.device, self.rank, self.world = device, rank, world
        self.ptr = None
        self._handle = (ctypes.c_uint8 * IPC_HANDLE_BYTES)()
        self._opened = []
        self._C = native.calls()

    def alloc(self, uncached):
        mb = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            self._C.mpc_mailbox_alloc(self.world, int(uncached), ctypes.byref(mb))
        self.ptr = mb.value
        if self.world > 1:
            self._C.mpc_ipc_handle(ctypes.c_void_p(self.ptr), self._handle)

    def connect(self, group):
        """The ranks' IPC handles exchanged over the group, every peer's mailbox
        opened, the pointers written into this mailbox's header."""
        ptrs = [0] * self.world
        ptrs[self.rank] = self.ptr
        if self.world > 1:
            local = torch.tensor(bytearray(self._handle), dtype=torch.uint8, device=self.device)
            handles = gather_bytes(local, group).cpu().numpy().reshape(self.world, -1)
        for r in range(self.world):
            if r == self.rank:
                continue
            p = ctypes.c_void_p()
            hr = (ctypes.c_uint8 * IPC_HANDLE_BYTES).from_buffer_copy(handles[r].tobytes())
            with torch.cuda.device(self.device):       # mapped for this rank's GPU
                self._C.mpc_ipc_open(hr, ctypes.byref(p))
            self._opened.append(p.value)
            ptrs[r] = p.value
        arr = (ctypes.c_void_p * self.world)(*ptrs)
        with torch.cuda.device(self.device):
            self._C.mpc_mailbox_set_peers(ctypes.c_void_p(self.ptr), self.rank, self.world, arr)

    def self_test(self):
        """mpc_mailbox_ping, once every rank's header is written: 1 if every
        peer's store arrived, 0 if the wait timed out."""
        flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._C.mpc_mailbox_ping(ctypes.c_void_p(self.ptr), 0x5A17, flag.data_ptr(),
                                     native.current_stream())
        return int(flag.item())

    def clear(self):
        self._C.mpc_mailbox_clear(ctypes.c_void_p(self.ptr), self.world, native.current_stream())

    def free(self):
        """Idempotent; a failing release is ignored (nothing left to do about it)."""
        L = native.lib()
        for p in self._opened:
            L.mpc_ipc_close(ctypes.c_void_p(p))
        self._opened = []
        if self.ptr:
            torch.cuda.synchronize()
            L.mpc_mailbox_free(ctypes.c_void_p(self.ptr))
            self.ptr = None


class DeviceEpisode:
    """The same episode with its state in HBM (mpc_episode_* C ABI): a step
    is enqueued without any host synchronisation, so the host only launches
    and the GPU runs steps back to back.  `read_log()` syncs and decodes the
    per-step records (and raises ChainError if a device wait timed out).

    Capturing chained / exchange steps into a hipGraph: end the captured
    sequence with `flush()` inside the capture.  A replay repeats the captured
    launches' epochs; the flush's update clears the published constants' tags,
    without it the next replay's launch with the last epoch could accept the
    previous replay's constants (include/mpc_rollout.h).

    obstacles / set_obstacles(): keep-out circles (x, y, r) in world
    coordinates, at most 16, with the semantics of the one-shot entries
    (mpc_rollout_partials_obstacles): a candidate that ends a step strictly
    inside one never wins; if all do, the step has no winner (MPC_EP_STALE).
    `n_blocked` (device int64) holds the blocked candidates of the last
    rollout.  Supported with circles: the two-launch step (split=True; sampler
    or caller controls, also expand() + advance() across ranks) and the
    one-GPU chained step (chain=True, SoA or tiled).  A chained tile block
    needs the step's pose before its rollout, so it waits for block 0 first:
    with circles the chained step gives up the overlap it exists for.  At
    config C it is still the faster form with 4 circles (40.3 against 43.4 us
    per step), level with 16 (65.6 / 65.7 us) and SLOWER than the two-launch
    step with one (40.4 against 39.7 us); counting n_blocked adds ~5 us to
    either.  Not supported, ValueError: generate,
    split=False, the chained exchange / P2P / overlapped steps, run().  With no
    circles every call is the one made without the feature.

    polygons / set_polygons(): convex keep-out polygons, each a sequence of 3
    to 8 (x, y) vertices in either orientation, at most 4, beside the circles
    and with the semantics of mpc_rollout_partials_keepout: strictly inside
    blocks, one blocked by a circle and a polygon counts once in `n_blocked`.
    The same step forms take them and the same ones refuse them; with no
    polygons every call is the one made without them.  As with circles the
    chained tile blocks wait for the step's pose first: at config C the
    chained step is the faster form with one polygon (44.7 against 46.3 us per
    step) and the slower one with four octagons (83.0 against 80.7 us)
    (DESIGN.md §5)."""

    def __init__(self, engine, n_cand_total, n_steps, rank=0, world=1, seed=20261015,
                 integrator="rect", group=None, start=(0.0, 0.0, 0.0, 0.0, 0.0), target=(2, 3),
                 log_capacity=4096, split=True, exchange=None, chain=False, L=None,
                 generate=False, max_steps=0, incumbent0=0.0, enumerate=False, overlap=False,
                 p2p=False, mailbox_uncached=True, obstacles=(), polygons=()):
        self.eng = engine
        self.lib = native.lib()           # entries that return their status (callers, tests)
        self._C = native.calls()          # entries that raise
        self.n_total = int(n_cand_total)
        self.n_steps = int(n_steps)
        self.rank, self.world, self.group = rank, world, group
        self.lo, self.hi = shard_range(self.n_total, rank, world)
        self.n_local = self.hi - self.lo
        self._shard = (self.n_local, self.n_steps, self.lo)
        self.integrator = integrator
        self.cfg = reference_episode_config(start, target, seed, max_steps=max_steps,
                                            incumbent0=incumbent0, enumerate=enumerate)
        if L is not None:                 # wheelbase other than config.py's (tests: L not 2^k)
            self.cfg.L = float(L)
        dev = engine.device
        self.state = torch.zeros(self.lib.mpc_episode_state_bytes(), dtype=torch.uint8,
                                 device=dev)
        self._head = (ctypes.byref(self.cfg), self.state.data_ptr())
        self.v_sc = torch.empty((self.n_steps, self.n_local), dtype=torch.float64, device=dev)
        self.b_sc = torch.empty_like(self.v_sc)
        self.local = torch.zeros(RESULT_BYTES, dtype=torch.uint8, device=dev)
        self.winner = torch.zeros(RESULT_BYTES, dtype=torch.uint8, device=dev)
        self.log_capacity = int(log_capacity)
        self.log = torch.zeros(self.log_capacity * LOG_BYTES, dtype=torch.uint8, device=dev)
        self._log_host = None             # pinned copy of the log (read_log)
        # zeroed: an exchange step's tagged block records must never find an
        # old allocation's bytes carrying a tag (mpc_exchange.h store_tagged_rec)
        self.ws = torch.zeros(self.lib.mpc_workspace_bytes(self.n_local, self.n_steps),
                              dtype=torch.uint8, device=dev)
        self._integ = INTEGRATORS[integrator]
        self.cur = (self.v_sc, self.b_sc)
        self.split = bool(split)
        # exchange: the multi-GPU step structure (finalize -> all_gather ->
        # advance).  Always on for world > 1; forcing it on one rank rehearses
        # the RCCL exchange (and its HIP-graph capture) on a single GPU.
        self.exchange = world > 1 if exchange is None else bool(exchange)
        if world > 1 and not self.exchange:
            raise ValueError("world > 1 needs the exchange step")
        # chain: each step's launch also completes the previous step
        # (caller-resident controls, aligned path); flush() completes the
        # last one.  The workspaces alternate.
        self.chain = bool(chain)
        self._ws = [self.ws, torch.zeros_like(self.ws)] if self.chain else [self.ws]
        self.generate = bool(generate)
        if (len(obstacles) or len(polygons)) and not self._takes_obstacles():
            raise ValueError(self._OBSTACLE_FORMS)
        # exchange + chain: this rank's best candidate of the step (the
        # all_gather payload of mpc_episode_exchange_step)
        self.cand = torch.zeros(CANDIDATE_BYTES, dtype=torch.uint8, device=dev)
        # overlap (exchange + chain): see _OverlappedChain
        self.overlap = bool(overlap)
        if self.overlap and not (self.exchange and self.chain):
            raise ValueError("overlap: the chained exchange step only (exchange=True, chain=True)")
        if self.overlap and self.world > 32:
            raise ValueError("overlap: at most 32 ranks (gathered candidates staged in LDS)")
        # p2p (exchange + chain): see _P2PChain and _p2p_setup, which falls
        # back to the all_gather exchange (p2p = False) if the mailboxes fail
        self.p2p = bool(p2p)
        if self.p2p and (self.overlap or not (self.exchange and self.chain)):
            raise ValueError("p2p: the chained exchange step (exchange=True, chain=True), "
                             "not overlapped")
        self._mailbox = None
        self.p2p_status = None
        if self.p2p:
            self._p2p_setup(dev, bool(mailbox_uncached))
        # the chained step structure, chosen once
        self._form = (_OneGpuChain() if not self.exchange else
                      _P2PChain(self._mailbox) if self.p2p else
                      _OverlappedChain(self.world, dev) if self.overlap else _GatheredChain())
        # generate: steps without caller controls draw their candidates inside
        # the rollout (mpc_episode_generate_step) instead of sampling them into
        # v_sc / b_sc first — the same candidates, never written to HBM
        if self.generate and self.exchange:
            raise ValueError("generated controls: one GPU (no exchange step)")
        self._gen_ws = None               # workspace of the generated step
        self._run_ws = None               # workspace of run()
        self._pending = None              # what the form's last launch left to complete
        self._epoch = 0
        self._checked = {}
        self.steps_enqueued = 0
        self.n_blocked = torch.zeros(1, dtype=torch.int64, device=dev)
        self._obs, self._n_obs = None, 0
        self._poly, self._n_poly = None, 0
        self.set_obstacles(obstacles)
        self.set_polygons(polygons)
        self.reset(_fresh_mailbox=True)

    _OBSTACLE_FORMS = ("keep-out circles and polygons: the two-launch step (split=True, "
                       "generate=False) and the one-GPU chained step (chain=True, "
                       "exchange=False) only")

    def set_obstacles(self, circles):
        """The keep-out circles of the steps enqueued from now on (a pending
        chained step is completed first; its rollout already ran under the
        previous circles)."""
        obs, n = make_obstacles(circles)
        if n > MPC_MAX_OBSTACLES:
            raise ValueError(f"at most {MPC_MAX_OBSTACLES} obstacles")
        if n and not self._takes_obstacles():
            raise ValueError(self._OBSTACLE_FORMS)
        if self._pending is not None:
            self.flush()
        self._obs, self._n_obs = obs, n

    @staticmethod
    def checked_polygons(polygons):
        """(MpcPolygon array or None, count) of the episode's polygons
        (make_polygons), ValueError for more than MPC_MAX_POLYGONS and for one
        the library's rule refuses (not strictly convex and simple)."""
        rows = [polygon_vertices(g) for g in (polygons or ())]
        if len(rows) > MPC_MAX_POLYGONS:
            raise ValueError(f"at most {MPC_MAX_POLYGONS} polygons")
        if not all(polygon_is_convex(g) for g in rows):
            raise ValueError("a keep-out polygon is strictly convex and simple: split a "
                             "non-convex or degenerate polygon into convex pieces")
        return make_polygons(rows)

    def set_polygons(self, polygons):
        """The keep-out polygons of the steps enqueued from now on (a pending
        chained step is completed first; its rollout already ran under the
        previous polygons)."""
        poly, n = self.checked_polygons(polygons)
        if n and not self._takes_obstacles():
            raise ValueError(self._OBSTACLE_FORMS)
        if self._pending is not None:
            self.flush()
        self._poly, self._n_poly = poly, n

    def _takes_obstacles(self):
        return self.split and not self.generate and not (self.chain and self.exchange)

    def _obstacle_args(self):
        """The hook of _entry: None (the base entries), or what their _obstacles
        twins take besides: (circles, count, n_blocked_out)."""
        if not self._n_obs:
            return None
        return self._obs, self._n_obs, self.n_blocked.data_ptr()

    def _polygon_args(self):
        """The second hook of _entry: None, or what the `_keepout` twins take
        after the circles: (polygons, count)."""
        if not self._n_poly:
            return None
        return self._poly, self._n_poly

    def _entry(self, name, head, *args):
        """The call site of the chained launch, the two-launch step and partials:
        entry `name`, or with circles its `_obstacles` twin, which takes them
        after `head` (up to the state) and n_blocked_out before the stream, or
        with polygons its `_keepout` twin, which takes them after the circles."""
        extra = self._obstacle_args()
        polys = self._polygon_args()
        if polys is not None:
            *circles, blocked = extra if extra is not None else (None, 0, self.n_blocked.data_ptr())
            twin = getattr(self._C, name + "_keepout")
            return twin(*head, *circles, *polys, *args[:-1], blocked, args[-1])
        if extra is None:
            return getattr(self._C, name)(*head, *args)
        *circles, blocked = extra
        twin = getattr(self._C, name + "_obstacles")
        return twin(*head, *circles, *args[:-1], blocked, args[-1])

    def _p2p_setup(self, dev, uncached):
        """The mailbox's three stages (_Mailbox), the ranks' verdict reduced
        after each; every rank issues the same reductions whatever fails
        locally.  If any rank fails any of it, every rank falls back to the
        all_gather exchange (self.p2p = False; the reason in self.p2p_status)."""
        if self.world > 32:
            raise ValueError("p2p: at most 32 ranks")
        self.p2p_status = "mailbox peer stores"
        mb = self._mailbox = _Mailbox(dev, self.rank, self.world)

        def tried(stage, *args):
            try:
                stage(*args)
                return 1
            except RuntimeError as e:
                self.p2p_status = f"fell back to all_gather: {e}"
                return 0

        ok = self._all_ranks(tried(mb.alloc, uncached), "min")
        ok = self._all_ranks(ok and tried(mb.connect, self.group), "min")
        if ok:      # every rank's header is written (the reduction above is a barrier)
            ok = mb.self_test()
            if not ok:
                self.p2p_status = "fell back to all_gather: the mailbox self-test timed out"
            ok = self._all_ranks(ok, "min")
        if not ok:
            if self.p2p_status == "mailbox peer stores":
                self.p2p_status = "fell back to all_gather: a peer's mailbox setup failed"
            mb.free()
            self._mailbox = None
            self.p2p = False

    def _all_ranks(self, value, op):
        """min / max over the ranks of an int (a collective: every rank calls it)."""
        if self.world == 1:
            return int(value)
        return reduce_int(value, op, self.group, self.state.device)

    def close(self):
        """Release the P2P mailbox and the peers' mappings, and let the
        overlapped form's side stream drain (idempotent).  Call it before the
        process group is destroyed: no collective or peer store of this
        episode may still be in flight when the process exits."""
        self._form.close()
        if self._mailbox is not None:
            self._mailbox.free()

    def reset(self, _fresh_mailbox=False):
        """Restart the episode from cfg.  P2P form: also zeroes this rank's
        mailbox slots (mpc_mailbox_clear), so that no step replayed with an
        epoch of the previous run (a graph captured before the reset) reads a
        stale candidate as fresh; with world > 1 that makes reset() a
        collective — every rank calls it, and none posts into a peer's
        mailbox before every rank has cleared its own.  (A new mailbox is
        zeroed by mpc_mailbox_alloc.)"""
        self._C.mpc_episode_reset(*self._head, native.current_stream())
        self.steps_enqueued = 0
        self._pending = None
        if self.p2p and self._mailbox.ptr and not _fresh_mailbox:
            self._mailbox.clear()
            if self.world > 1:
                torch.cuda.current_stream().synchronize()
                self._all_ranks(1, "min")      # every rank cleared

    def _tail(self):            # (_head, _shard and this: argument groups the entries share)
        return self.log.data_ptr(), self.log_capacity, native.current_stream()

    def _prev_ptrs(self, pend):
        return self._ptrs(pend)[:2] if pend is not None else (None, None)

    def _ptrs(self, controls):
        """(v pointer, beta pointer, integrator id) of a checked control batch:
        SoA (v, beta) or a tiled tensor (MPC_LAYOUT_TILED: beta = v + 512)."""
        if _is_tiled(controls):
            p = controls.data_ptr()
            return p, p + 8 * MPC_TILE, self._integ | MPC_LAYOUT_TILED
        v, b = controls
        return v.data_ptr(), b.data_ptr(), self._integ

    def _seen(self, key, *tensors):
        """Was this very batch (same tensor objects) checked before?  The cache
        holds weak references only: a caller's per-step batches are not kept
        alive by it (and a new tensor reusing a freed one's id and memory is
        not mistaken for it)."""
        refs = self._checked.get(key)
        return refs is not None and all(r() is t for r, t in zip(refs, tensors))

    def _remember(self, key, *tensors):
        if len(self._checked) >= 4096:
            self._checked = {k: r for k, r in self._checked.items()
                             if all(x() is not None for x in r)}
            if len(self._checked) >= 4096:
                self._checked.clear()
        self._checked[key] = tuple(weakref.ref(t) for t in tensors)

    def _check_controls(self, controls):
        if _is_tiled(controls):
            return self._check_tiled(controls)
        v, b = controls
        key = (id(v), id(b), v.data_ptr(), b.data_ptr())
        if self._seen(key, v, b):        # a resident batch seen before: checked once
            return v, b
        if (tuple(v.shape) != (self.n_steps, self.n_local) or v.shape != b.shape
                or v.dtype != torch.float64 or b.dtype != torch.float64
                or not v.is_contiguous() or not b.is_contiguous()
                or v.device != self.v_sc.device or b.device != self.v_sc.device):
            raise ValueError("controls must be contiguous float64 [n_steps, n_local] "
                             "tensors on the episode's device")
        self._remember(key, v, b)
        return v, b

    def _check_tiled(self, t):
        key = (id(t), t.data_ptr())
        if self._seen(key, t):
            return t
        if (tuple(t.shape) != (-(-self.n_local // MPC_TILE), self.n_steps, 2, MPC_TILE)
                or t.dtype != torch.float64 or not t.is_contiguous()
                or t.device != self.v_sc.device or t.data_ptr() % 16):
            raise ValueError("tiled controls must be a contiguous 16-B aligned float64 "
                             "[ceil(n_local / 512), n_steps, 2, 512] tensor on the episode's "
                             "device (Expansion.sample_controls_tiled)")
        self._remember(key, t)
        return t

    def _chain_step(self, controls, events=None):
        """One chained launch: this step's rollout + the previous step's
        completion (one GPU: finalize + update; multi-GPU: selection over the
        ranks' candidates + update), in the episode's step structure."""
        form = self._form
        ctl = self._check_controls(controls)
        tiled = _is_tiled(ctl)
        if tiled and not form.pends_controls:
            raise ValueError("tiled controls: the one-GPU and P2P chained steps only")
        self.cur = ctl
        pend = self._pending
        if form.pends_controls and pend is not None and _is_tiled(pend) != tiled:
            raise ValueError("a chained episode keeps one control layout until its flush")
        if events:
            events[0].record()
        self._pending = form.launch(self, ctl, pend, events)
        if pend is not None:
            self.steps_enqueued += 1
        self._ws.reverse()

    def run(self, batches):
        """len(batches) COMPLETE MPC steps in one persistent launch per 64
        (mpc_episode_run, csrc/mpc_run.h): step j over batches[j] — each a
        resident SoA (v, beta) pair or a tiled tensor, one layout for the run.
        One GPU, rect+cum, the chained step's controls; the log, the state and
        `local` (the last step's winner) equal those of the same chained steps
        and their flush, bit for bit.  A pending chained step is completed
        first."""
        if self.exchange:
            raise ValueError("the persistent run: one GPU (no exchange step)")
        if self._n_obs or self._n_poly:
            raise ValueError("run(): " + self._OBSTACLE_FORMS)
        if self.integrator != "rect+cum" or self.n_local % 2:
            raise ValueError("the persistent run streams rect+cum candidates, n_local even")
        batches = list(batches)
        if not batches:
            return
        self.flush()
        ctls = [self._check_controls(c) for c in batches]
        tiled = _is_tiled(ctls[0])
        if any(_is_tiled(c) != tiled for c in ctls):
            raise ValueError("one control layout per run")
        if not tiled and any(not self._chainable(c) for c in ctls):
            raise ValueError("SoA controls of a run must be 16-B aligned")
        ptrs = [self._ptrs(c) for c in ctls]
        k = len(ptrs)
        V = (ctypes.c_void_p * k)(*[p[0] for p in ptrs])
        B = (ctypes.c_void_p * k)(*[p[1] for p in ptrs])
        if self._run_ws is None:
            # zeroed once; every run leaves it zeroed (tagged records consumed)
            self._run_ws = torch.zeros(self.lib.mpc_episode_run_workspace_bytes(self.n_local),
                                       dtype=torch.uint8, device=self.state.device)
        # k consecutive nonzero epochs (the published constants' tags)
        if self._epoch + k >= 0xFFFFFFF0:
            self._epoch = 0
        e0 = self._epoch + 1
        self._epoch += k
        self._C.mpc_episode_run(
            *self._head, e0, V, B, k, *self._shard, ptrs[0][2], self._run_ws.data_ptr(),
            self._run_ws.numel(), self.local.data_ptr(), *self._tail())
        self.cur = ctls[-1]
        self.steps_enqueued += k

    def _next_epoch(self):
        # nonzero, differs from the last and in parity (the P2P mailbox's two
        # slots alternate: 0xFFFFFFFE is followed by 1)
        self._epoch = self._epoch % 0xFFFFFFFE + 1
        return self._epoch

    def flush(self):
        """Complete the step a chained launch left pending (no-op otherwise)."""
        pend, self._pending = self._pending, None
        if pend is None:
            return
        self._form.flush(self, pend)
        self.steps_enqueued += 1

    def chain_error(self, local=False):
        """EpisodeState::chain_error — with world > 1 the MAX over the ranks (a
        collective: every rank calls it), since a rank whose wait timed out
        posted nothing, so its peers' steps diverge from the true arg-min
        while their own code stays 0.  local=True: this rank's code only."""
        e = ctypes.c_int32(0)
        self._C.mpc_episode_chain_error(self.state.data_ptr(), ctypes.byref(e),
                                        native.current_stream())
        return int(e.value) if local else self._all_ranks(e.value, "max")

    def _generate_step(self, events):
        """One complete step on candidates drawn inside the rollout."""
        if self._gen_ws is None:
            self._gen_ws = torch.empty(self.lib.mpc_episode_generate_workspace_bytes(
                self.n_local, self.n_steps), dtype=torch.uint8, device=self.state.device)
        if events:
            events[0].record()
        self._C.mpc_episode_generate_step(
            *self._head, *self._shard, self._integ, self._gen_ws.data_ptr(),
            self._gen_ws.numel(), self.local.data_ptr(), *self._tail())
        _stop(events)
        self.steps_enqueued += 1

    def expand(self, events=None, controls=None):
        """Grid + sampler + rollout + finalize for this rank's shard.
        controls: optional caller-resident (v_sc, beta_sc) fp64 [n_steps,
        n_local] for this step — the rollout streams them instead of the
        sampler's (the candidate set is the caller's input).
        events: optional (start, stop) torch.cuda.Event pair recorded around
        the rollout (+ selection) launch."""
        C, st = self._C, native.current_stream()
        self.flush()
        if controls is None and self.generate:
            return self._generate_step(events)
        if controls is None:
            C.mpc_episode_sample(*self._head, self.v_sc.data_ptr(), self.b_sc.data_ptr(),
                                 *self._shard, st)
            self.cur = (self.v_sc, self.b_sc)
        else:
            self.cur = self._check_controls(controls)
        one_gpu = not self.exchange  # one GPU: the step's launch also advances the episode
        args = (self.state.data_ptr(), self.cur[0].data_ptr(), self.cur[1].data_ptr(),
                *self._shard, self._integ, self.ws.data_ptr(), self.ws.numel(),
                self.local.data_ptr(),
                ctypes.byref(self.cfg) if one_gpu else None,
                self.log.data_ptr() if one_gpu else None, self.log_capacity if one_gpu else 0, st)
        if events:
            events[0].record()
        if self.split and not events:
            # streaming kernel, then the selection kernel: two launches in one
            # host call (the faster form on MI355X: 44.8 vs 47.5 us per
            # config-C step than the one-launch form below); with circles
            # (split, checked by set_obstacles) the rollout tests them
            self._entry("mpc_episode_step", args[:1], *args[1:])
        elif self.split:
            self.partials(st)
            C.mpc_episode_finalize(*args)
        else:
            # one launch: the last block to finish runs the selection
            C.mpc_episode_rollout(*args)
        _stop(events)
        if one_gpu:
            self.steps_enqueued += 1

    def partials(self, st=None):
        """The streaming rollout/arg-min kernel alone on the current controls
        (writes only the workspace block records; the episode is unchanged)."""
        self.flush()
        if _is_tiled(self.cur):
            raise ValueError("the streaming kernel alone reads SoA controls")
        v, b = self.cur
        st = st if st is not None else native.current_stream()
        self._entry("mpc_episode_partials", (self.state.data_ptr(),), v.data_ptr(), b.data_ptr(),
                    self.n_local, self.n_steps, self._integ, self.ws.data_ptr(), self.ws.numel(), st)

    def advance(self):
        """Multi-GPU: all_gather of the per-rank winners (RCCL) + selection +
        episode update in one launch; no host synchronisation.  (On one GPU
        the update already ran inside finalize.)"""
        if not self.exchange:
            return
        gathered = gather_results(self.local, self.group)
        self._C.mpc_episode_advance(*self._head, gathered.data_ptr(), self.world, *self._tail())
        self.steps_enqueued += 1

    def step(self, events=None, controls=None):
        """One MPC step.  controls: this step's resident candidates — SoA
        (v_sc, beta_sc) [n_steps, n_local] or, for the chained steps (one GPU or
        P2P), a tiled tensor (Expansion.sample_controls_tiled); None: the
        device sampler draws them."""
        if self.chain and controls is not None and self._chainable(controls):
            self._chain_step(controls, events)
            return
        if controls is not None and _is_tiled(controls):
            raise ValueError("tiled controls: chained rect+cum steps only (chain=True)")
        self.expand(events, controls)
        self.advance()

    def _chainable(self, controls):
        if self.integrator != "rect+cum" or self.n_local % 2:
            return False
        return _is_tiled(controls) or (controls[0].data_ptr() % 16 == 0
                                       and controls[1].data_ptr() % 16 == 0)

    def read_log(self):
        """Complete any pending step, sync, and decode the per-step records.
        Raises ChainError if a chained / exchange step's bounded device wait
        timed out on ANY rank (chain_error(), reduced over the ranks): such a
        step ran on speculated constants or dropped a rank's candidate, so
        the log records must not be trusted.  With world > 1 every rank must
        call it (the reduction is a collective)."""
        self.flush()
        torch.cuda.current_stream().synchronize()
        err = self.chain_error()
        if err:
            raise ChainError(err)
        # the log is complete: one copy into pinned host memory (a staged copy
        # to pageable memory left an async-copy completion callback undelivered
        # at process exit under rocprofv3's memory-copy tracing,
        # profiles/r06/overlap_exit/)
        if self._log_host is None:
            self._log_host = torch.empty(self.log.numel(), dtype=torch.uint8).pin_memory()
        self._log_host.copy_(self.log, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        raw = self._log_host.numpy().tobytes()
        n = min(self.steps_enqueued, self.log_capacity)
        recs = [MpcEpisodeLog.from_buffer_copy(raw[i * LOG_BYTES:(i + 1) * LOG_BYTES])
                for i in range(self.log_capacity)]
        # a written record has episode >= 1 (slots never written are zero)
        recs = [r for r in recs if r.episode >= 1 and r.step < self.steps_enqueued]
        recs.sort(key=lambda r: r.step)
        return recs[-n:]
