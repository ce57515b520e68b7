"""Sharded detect -> refine -> uplift worker (one process per GPU) and the single collective of the path.

The reference is single-process / single-GPU.  The path shards over independent units:
video streams (or frame ranges of one stream with a 1-frame halo, because triple t needs frames t..t+2) and
trajectories.  Weights are replicated; there is no data-path collective.  The only exchange is the final gather
of small fixed-size records -- per frame (x, y, visibility) float64 and per trajectory (spin[3], T', pos[T,3])
float32 -- a few KB per stream, latency-bound on any xGMI topology (``gather_records``).
"""
import numpy as np
import torch

from . import _lib, wasb

TRAJ_LEN_DEFAULT = 32


def shard_range(n_units, world, rank):
    """Contiguous balanced partition of range(n_units): the first n_units % world ranks get one extra unit."""
    if world <= 0 or not (0 <= rank < world):
        raise ValueError('bad world/rank %d/%d' % (world, rank))
    q, r = divmod(n_units, world)
    start = rank * q + min(rank, r)
    return start, start + q + (1 if rank < r else 0)


def frame_range_with_halo(n_frames, world, rank):
    """Split ONE stream of n_frames (n_frames-2 triples) over ranks.  Returns (first_frame, last_frame_exclusive,
    first_triple, n_triples): each rank reads its triples' frames plus the 2-frame look-ahead."""
    t0, t1 = shard_range(max(n_frames - 2, 0), world, rank)
    if t1 <= t0:
        return 0, 0, t0, 0
    return t0, t1 + 2, t0, t1 - t0


def _pack_records(records, spec, device):
    """One byte buffer per rank: int64 row counts of every key (sorted), then each key's rows in a region of fixed capacity."""
    keys = sorted(spec)
    cap = {k: int(spec[k][0]) * int(np.prod(spec[k][1], dtype=np.int64)) * torch.empty((), dtype=spec[k][2]).element_size() for k in keys}
    total = 8 * len(keys) + sum(cap.values())
    buf = torch.zeros((total,), dtype=torch.uint8, device=device)
    rows = []
    off = 8 * len(keys)
    for k in keys:
        v = records[k].contiguous()
        if v.dtype != spec[k][2] or tuple(v.shape[1:]) != tuple(spec[k][1]) or v.shape[0] > spec[k][0]:
            raise ValueError('record %r %s/%s does not fit its spec %s' % (k, tuple(v.shape), v.dtype, spec[k]))
        rows.append(v.shape[0])
        nb = v.numel() * v.element_size()
        if nb:
            buf[off:off + nb] = v.to(device).reshape(-1).view(torch.uint8)
        off += cap[k]
    buf[:8 * len(keys)] = torch.tensor(rows, dtype=torch.int64).view(torch.uint8).to(device)
    return buf, keys, cap


def _unpack_records(flat, world, keys, cap, spec):
    total = flat.numel() // world
    out = {k: [] for k in keys}
    for r in range(world):
        b = flat[r * total:(r + 1) * total]
        rows = b[:8 * len(keys)].clone().view(torch.int64).tolist()
        off = 8 * len(keys)
        for k, n in zip(keys, rows):
            shape, dt = tuple(spec[k][1]), spec[k][2]
            nb = n * int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dt).element_size()
            out[k].append(b[off:off + nb].clone().view(dt).reshape((n,) + shape))
            off += cap[k]
    return out


def gather_records(records, dist=None, dst=0, spec=None):
    """The one exchange of the path: gather a dict of per-rank records -- tensors whose first dimension may differ per
    rank -- on rank `dst`.  Returns {key: [tensor_of_rank0, tensor_of_rank1, ...]} on dst, None elsewhere; with dist=None (single
    process) it just wraps the local records.

    `spec` = {key: (max_rows, row_shape, dtype)} (StreamWorker.record_spec()) fixes every key's capacity, so a step is exactly ONE
    collective: all ranks contribute one equally sized byte buffer (row counts + rows) to an all_gather.  Without a spec the
    capacities are agreed first (one extra all_reduce of the row counts): two collectives.  nccl (= RCCL) gathers device buffers,
    gloo (CPU tests, single-GPU dry runs) host buffers.  With world > 1 the tensors returned on `dst` are HOST tensors (the
    gathered payload is a few KB of results that the caller reads on the host); with one process the local records are returned as
    they are."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return {k: [v] for k, v in records.items()}
    world, rank = dist.get_world_size(), dist.get_rank()
    on_host = dist.get_backend() == 'gloo'
    any_v = next(iter(records.values()))
    device = torch.device('cpu') if on_host else any_v.device
    if spec is None:
        keys = sorted(records)
        rows = torch.tensor([records[k].shape[0] for k in keys], dtype=torch.int64, device=device)
        dist.all_reduce(rows, op=dist.ReduceOp.MAX)
        spec = {k: (max(int(n), 1), tuple(records[k].shape[1:]), records[k].dtype) for k, n in zip(keys, rows.tolist())}
    buf, keys, cap = _pack_records(records, spec, device)
    flat = torch.empty((world * buf.numel(),), dtype=torch.uint8, device=device)
    dist.all_gather_into_tensor(flat, buf)
    if rank != dst:
        return None
    return _unpack_records(flat.cpu(), world, keys, cap, spec)


class StreamWorker:
    """Per-GPU worker: owns one CNN handle, one uplift handle, and runs whole clips through the path.
    Raises RuntimeError without a HIP device (no CPU fallback).

    Certified argmax (`certify=True`, bf16): eps is calibrated on the first clip and audited while the worker runs by `cert`
    (wasb.EpsAudit, where the protocol is described); `audit` reports the counts, `audit_every=0` switches the strip audit off.  The
    worker adds its own policy: audit crops, the crop budget, the margin log, its streams and pinned buffers."""

    def __init__(self, device, wasb_state_dict, uplift_state_dict, net_wh=(1280, 704), max_triples=256, uplift_size='large',
                 traj_len=TRAJ_LEN_DEFAULT, seq_len=50, dtype='bf16', certify=True, audit_every=256, audit_seed=0, exact_windows=False,
                 audit_every_fast=64, audit_settle_clips=8, audit_crops_every=16):
        from . import glue, refine, uplift, _lib
        _lib.require_gpu()
        self._glue, self._refine, self._uplift, self._lib = glue, refine, uplift, _lib
        self.device = torch.device(device)
        self.net_w, self.net_h = net_wh
        self.traj_len, self.seq_len = traj_len, seq_len
        self.max_triples = max_triples
        self.net = wasb.WASBNet(wasb_state_dict, resolution=net_wh, max_batch=max_triples, dtype=dtype, device=self.device)
        self.max_segments = max(64, (max_triples + traj_len - 1) // traj_len)
        self.up = uplift.get_model('connectstage', uplift_size, 'dynamic', 'new', state_dict=uplift_state_dict,
                                   max_batch=self.max_segments, max_len=seq_len, device=self.device)
        # certified argmax (the fp32 path's indices from the bf16 path, csrc/certify.hip): calibrated on the first clip seen
        self.certify = bool(certify) and dtype == 'bf16'
        self.exact_windows = bool(exact_windows)
        # Strip audit rate, ADAPTIVE: `audit_every_fast` until `audit_settle_clips` clips in a row passed without a widening, then
        # `audit_every`.  New content is where a too-small eps is found (the soaks widen within the first clips of a content change).
        self.audit_every = int(audit_every)
        self.audit_every_fast = min(int(audit_every_fast), self.audit_every) if int(audit_every_fast) > 0 else self.audit_every
        self.audit_settle_clips = int(audit_settle_clips)
        self.cert = wasb.EpsAudit(self.net, every=self.audit_every if self.certify else 0, every_fast=self.audit_every_fast,
                                  settle_clips=self.audit_settle_clips, seed=audit_seed)
        # Audit crops (round 6): one single-candidate heatmap per `audit_crops_every` triples gets an fp32 crop although its index is
        # already certain; the crop reports |bf16 - fp32| at the winner.  The strip audit sees every pixel of a quarter-width strip of
        # one triple per 64-256; this sees ONE pixel -- the one the detection rests on -- of one triple per 16, at 0.1 ms each
        # (1.3 % of a step).  The phase is drawn per pass.  0 = off.
        self.audit_crops_every = int(audit_crops_every)
        self.audit_crop_frames = 0
        self._rng_crops = np.random.default_rng(audit_seed + 1)
        self._crop_hist = []          # crops asked for by the last passes (`_size_crop_budget`)
        # measurement (bench.py `ambiguous_share`): when set to a list, every collected clip appends the fp32 top-2 margins of its
        # heatmaps (`WASBNet.certify_margins`: +inf for single-candidate heatmaps)
        self.margin_log = None
        self._sub = None              # submit's two alternating streams (`submit_streams`)
        self._side = None             # collect's uplift stream
        self._pin_pool = {}           # pinned host buffers of the clips in flight (`_pinned`)

    @property
    def certify_eps(self):
        """eps of the certified argmax (the handle's): None until calibrated, or with certify off."""
        return self.cert.eps

    @certify_eps.setter
    def certify_eps(self, eps):          # (a widening by hand, e.g. `worker.certify_eps = worker.net.widen_eps(err)`)
        if eps != self.cert.eps:
            self.net.set_certify(eps)

    # the strip audit's pick rng and its quiet-clip count live in `cert` (tests steer them through the worker)
    _rng = property(lambda self: self.cert.rng, lambda self, rng: setattr(self.cert, 'rng', rng))
    _quiet_clips = property(lambda self: self.cert.quiet, lambda self, n: setattr(self.cert, 'quiet', n))
    fp32_reruns = property(lambda self: self.cert.fp32_reruns)
    recertified_clips = property(lambda self: self.cert.recertified_calls)
    recertified_heatmaps = property(lambda self: self.cert.recertified_heatmaps)

    def record_spec(self):
        """Capacities of the per-clip records (`gather_records(..., spec=...)`: one collective per step)."""
        return {'xyv': (self.max_triples, (3,), torch.float64), 'spin': (self.max_segments, (3,), torch.float32),
                'pos3d': (self.max_segments, (self.seq_len, 3), torch.float32), 'n_valid': (self.max_segments, (), torch.int64)}

    @property
    def audit(self):
        """{'audited_frames', 'max_err_seen', 'widened', 'eps', 'max_err_over_eps', 'recertified_clips'} of the certified argmax."""
        a = dict(self.net.audit_state)
        a['eps'] = self.certify_eps
        a['max_err_over_eps'] = (a['max_err_seen'] / self.certify_eps) if self.certify_eps else None
        a['recertified_clips'] = self.recertified_clips
        a['recertified_heatmaps'] = self.recertified_heatmaps
        # what the side-stream audit has covered: audited triples (calibration frames included) / triples processed.  A frame whose
        # error exceeds eps while no audited frame's does is missed with probability 1 - (the audit rate at that time) by the strip
        # audit (the candidate-level audit still sees it when it needs a crop): the guarantee is statistical and this is its rate
        a['frames_seen'] = self.cert.seen
        # strip audits (every pixel of a strip of the triple, calibration frames included) + audit crops (the winner's pixel of the triple)
        a['audit_crop_frames'] = self.audit_crop_frames
        a['strip_audited_share'] = (a['audited_frames'] / a['frames_seen']) if a['frames_seen'] else None
        a['audited_share'] = ((a['audited_frames'] + self.audit_crop_frames) / a['frames_seen']) if a['frames_seen'] else None
        a['audit_every_now'] = self.audit_rate()
        a['quiet_clips'] = self.cert.quiet
        a['widen_sources'] = dict(self.cert.widen_sources)
        return a

    def audit_rate(self):
        """Triples per audited triple right now (0 = side-stream audit off)."""
        return self.cert.rate()

    def detect(self, frames_u8):
        """(N,h,w,3) uint8 on the device -> (N-2,3) float64 [x, y, visibility] in 1920x1080 px (table-variant refine,
        like interface.py:116)."""
        return self._detect_blocking(frames_u8)

    def _xyv(self, idx, win):
        return self._refine.refine_windows_device(idx, win, self.net_h, self.net_w, 1920, 1080, self._lib.REFINE_TABLE)

    def _pass(self, frames_u8, counted=False):
        """Enqueue one detector pass over a clip -> (xyv, wasb.CertCall, audit ticket or None): the clip's strip audit on a side stream
        and its audit crops, then the forward with its status / info behind it (`EpsAudit.enqueue`).  counted=True: a whole-clip re-run
        after eps grew past the guard factor -- the same triples again, so they are not counted and no strip audit is drawn a second
        time (a new crop phase is)."""
        n = frames_u8.shape[0] - 2
        if self.certify and not self.net.certified:
            self.net.calibrate(frames_u8, n=8, exact_windows=self.exact_windows)
        audit = None if counted else self.cert.audit(self.cert.picks(n), frames_u8)
        if self.certify and self.audit_crops_every > 0:
            every = self.audit_crops_every
            phase = int(self._rng_crops.integers(every))
            self.net.certify_audit_crops(every, phase)
            if not counted:
                self.audit_crop_frames += len(range((-phase) % every, n, every))          # frames f < n with (f + phase) % every == 0
        if self.certify:
            self._size_crop_budget()
        call = self.cert.enqueue(frames_u8)
        return self._xyv(call.idx, call.win), call, audit

    def _size_crop_budget(self):
        """Crop budget of the next pass (it sizes the number of fp32 passes a call provisions; an unused pass still costs its launches):
        one and a half times the most any of the last eight passes asked for (+ slack) -- content that alternates between easy and hard
        clips keeps the hard clips' budget (twice the LAST clip's count sent 40 % of a hard clip that followed an easy one to the
        full-frame fp32 path); clips that outgrow it are flagged and repaired.  Before the first pass has settled: the handle's default."""
        if self._crop_hist:
            self.net.certify_budget(3 * max(self._crop_hist) // 2 + 16)

    def _settle(self, call, frames_u8, audit):
        """`EpsAudit.settle` of one pass -> True when its indices / windows changed.  A whole-clip re-run is a counted `_detect_blocking`."""
        self._crop_hist = (self._crop_hist + [self.net.decode_info(call.info)[0]])[-8:]
        rerun = lambda c: wasb.CertCall(c.f0, c.f1, *self._detect_blocking(frames_u8, full=True, counted=True)[1:])          # noqa: E731
        return bool(self.cert.settle([call], frames_u8, audit=audit, rerun=rerun))

    def _detect_blocking(self, frames_u8, full=False, counted=False):
        """One clip start to finish, blocking: (xyv device tensor) whose every index is certified under the current eps; full=True:
        (xyv, idx, win, host status 0/1/2) of the pass that produced it.  counted=True: see `_pass`."""
        xyv, call, audit = self._pass(frames_u8, counted)
        if call.status is not None and self._settle(call, frames_u8, audit):
            xyv = self._xyv(call.idx, call.win)
        return (xyv, call.idx, call.win, None if call.status is None else call.status & _lib.CERT_STATUS_MASK) if full else xyv

    def uplift_segments(self, positions, table_px, fps):
        """Cut the detections into rallies of `traj_len` frames, filter / normalise / pad each like the reference
        (inference/utils.py:70-102, :268-309) and run them as one uplift batch.
        Returns (spin_local (S,3), pos3d (S,seq_len,3), n_valid (S,)) on the device."""
        balls, tables, times, masks = [], [], [], []
        for s in range(0, positions.shape[0], self.traj_len):
            seg = positions[s:s + self.traj_len]
            filt, _, t = self._glue.filter_trajectory_ball(seg, seg, fps)
            b, tb, tm, mk = self._glue._uplifting_transform(filt, table_px, t, self.seq_len)
            balls.append(b); tables.append(tb); times.append(tm); masks.append(mk)
        mask = torch.cat(masks)
        rot, p3 = self.up(torch.cat(balls), torch.cat(tables), mask, torch.cat(times))
        spin = self._uplift.transform_rotationaxes(rot, p3)
        return spin, p3, mask.sum(1).to(torch.int64).to(self.device)

    def process_clip(self, frames_u8, table_px, fps):
        xyv = self._detect_blocking(frames_u8)
        spin, p3, nvalid = self.uplift_segments(xyv.cpu().numpy(), table_px, fps)
        return {'xyv': xyv, 'spin': spin, 'pos3d': p3, 'n_valid': nvalid}

    # Two-phase form of process_clip for back-to-back clips: `submit` only enqueues the detector (and an asynchronous copy
    # of its (N,3) result into pinned host memory) and returns at once; `collect` waits for that copy, runs the host glue
    # and enqueues the uplift.  Submitting clip k+1 before collecting clip k keeps the GPU busy while the host filters
    # and pads the detections of clip k.
    def submit(self, frames_u8):
        # consecutive clips are issued on two alternating streams: the fp32 crop passes of the certified argmax (the handle's own
        # stream, behind clip k's bf16 pass) then overlap with the bf16 micro-batches of clip k+1 instead of delaying them
        subs = self.submit_streams()
        sub = subs['streams'][subs['next']]
        subs['next'] ^= 1
        sub.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(sub):
            return self._submit(frames_u8, sub)

    def submit_streams(self):
        """The two alternating streams `submit` issues clips on (created on first use; callers that are about to create other
        streams -- a process group -- call this first so that the worker's stream-to-queue mapping does not depend on them)."""
        if self._sub is None:
            self._sub = {'streams': [torch.cuda.Stream(self.device), torch.cuda.Stream(self.device)], 'next': 0}
        return self._sub

    def _pinned(self, key, like):
        """A pinned host buffer shaped like `like` from the worker's pool (returned to it by collect): any number of clips may be
        in flight between submit and collect."""
        free = self._pin_pool.setdefault((key, tuple(like.shape), like.dtype), [])
        return free.pop() if free else torch.empty(like.shape, dtype=like.dtype, pin_memory=True)

    def _unpin(self, key, buf):
        if buf is not None:
            self._pin_pool[(key, tuple(buf.shape), buf.dtype)].append(buf)

    def _submit(self, frames_u8, sub):
        xyv, call, audit = self._pass(frames_u8)          # (the strip audit shares the GPU with this clip's detector pass)
        margin = self.net.certify_margins(call.idx.shape[0]) if call.status is not None and self.margin_log is not None else None
        dev = [xyv, call.idx, call.win, frames_u8]
        host = self._pinned('xyv', xyv)
        host.copy_(xyv, non_blocking=True)
        st_host = info_host = mg_host = None
        if call.status is not None:
            dev += [call.status, call.info]
            st_host = self._pinned('status', call.status)
            st_host.copy_(call.status, non_blocking=True)
            info_host = self._pinned('info', call.info)
            info_host.copy_(call.info, non_blocking=True)
            call.status, call.info = st_host, info_host
        if margin is not None:
            mg_host = self._pinned('margin', margin)
            mg_host.copy_(margin, non_blocking=True)
            margin.record_stream(sub)
        done = torch.cuda.Event()
        done.record()
        for t in dev:
            t.record_stream(sub)
        return {'call': call, 'margin': mg_host, 'xyv': xyv, 'host': host, 'done': done, 'frames': frames_u8, 'idx': call.idx, 'win': call.win,
                'status': st_host, 'info': info_host, 'stream': sub, 'audit': audit}

    def collect(self, ticket, table_px, fps):
        ticket['done'].synchronize()
        torch.cuda.current_stream(self.device).wait_stream(ticket['stream'])
        call = ticket['call']
        status_host = None
        if call.status is not None:
            # a clip certified under an eps that an audit has since found too small is re-certified here (wasb.EpsAudit.settle); the
            # ticket then describes the pass that produced its detections (indices, windows, status), not the stale one
            if self._settle(call, ticket['frames'], ticket['audit']):
                ticket['xyv'] = self._xyv(call.idx, call.win)
                ticket['host'].copy_(ticket['xyv'])
            ticket['idx'], ticket['win'] = call.idx, call.win
            status_host = call.status & _lib.CERT_STATUS_MASK          # 0 / 1 / 2 (guard bit dropped)
        # the uplift (about a hundred small launches for a handful of trajectories) runs on a side stream, so it shares
        # the GPU with the detector of the clip submitted in the meantime instead of queueing behind it
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        with torch.cuda.stream(self._side):
            spin, p3, nvalid = self.uplift_segments(ticket['host'].numpy(), table_px, fps)
        self._side.synchronize()
        # the results were allocated under the side stream and are consumed on the caller's stream (gather_records, RCCL,
        # user code): tell the caching allocator, so their blocks are not handed to the next clip's side-stream uplift
        # while reads queued on the caller's stream are still pending
        cur = torch.cuda.current_stream(self.device)
        for t in (spin, p3, nvalid):
            t.record_stream(cur)
        if ticket.get('margin') is not None and self.margin_log is not None:
            self.margin_log.append(ticket['margin'].numpy().copy())
        for k in ('host', 'status', 'info', 'margin'):
            self._unpin('xyv' if k == 'host' else k, ticket.get(k))
            ticket[k] = None
        ticket['call'] = None          # (its status viewed a pinned buffer that is back in the pool)
        ticket['status_host'] = status_host
        return {'xyv': ticket['xyv'], 'spin': spin, 'pos3d': p3, 'n_valid': nvalid, 'status': status_host}

    RECORD_KEYS = ('xyv', 'spin', 'pos3d', 'n_valid')          # what a step hands to gather_records

    def queue_groups(self, cycles=20_000_000):
        """Which of the worker's streams share a hardware queue: HIP maps the streams of a process onto GPU_MAX_HW_QUEUES (4)
        queues in the order in which they are first used, kernels of two streams on one queue do not overlap, and the pipeline's
        throughput moves by up to 6 % with the grouping.  Pairwise probes with two spin kernels (co-resident when both
        take the time of one).  Returns a canonical string, e.g. 'submit0+lane1 | submit1+crops | lane0 | audit+default'; every rank
        of a multi-GPU run should report the same one (bench.py gathers them).  Takes a few hundred milliseconds; idle GPU assumed."""
        dev = self.device
        named = [('submit%d' % k, s) for k, s in enumerate(self.submit_streams()['streams'])]
        ints = self.net.internal_streams()
        n_lanes = len(ints) - (1 if self.net.certified else 0)
        named += [('lane%d' % k, s) for k, s in enumerate(ints[:n_lanes])] + [('crops', s) for s in ints[n_lanes:]]
        if self.cert.audit_stream is not None:
            named.append(('audit', self.cert.audit_stream))
        if self._side is not None:
            named.append(('uplift', self._side))
        named.append(('default', torch.cuda.default_stream(dev)))

        def spin_ms(streams):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            cur = torch.cuda.current_stream(dev)
            e0.record(cur)
            for st in streams:
                st.wait_event(e0)
                with torch.cuda.stream(st):
                    torch.cuda._sleep(cycles)
                ev = torch.cuda.Event()
                ev.record(st)
                cur.wait_event(ev)
            e1.record(cur)
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1)
        one = spin_ms([named[0][1]])
        groups = []
        for name, st in named:
            for g in groups:
                if spin_ms([g[0][1], st]) > 1.6 * one:
                    g.append((name, st))
                    break
            else:
                groups.append([(name, st)])
        return ' | '.join('+'.join(n for n, _ in g) for g in groups)
