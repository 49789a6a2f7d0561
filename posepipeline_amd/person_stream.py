"""Streaming form of PersonBbox -> TopDownPerson -> LiftingPerson for every followed track id (host logic only).

The reference runs the three tables one after the other over the whole clip for ONE annotated subject
(`PersonBboxValid.keep_tracks`, pose_pipeline/pipeline.py:637-687, 1017-1095, 1259-1416).  `PersonStreams` produces the
same values for `keep_tracks = [tid]`, for every followed `tid`, while frames arrive in chunks:

  * the person box of frame t is the track's box iff exactly one row of the frame carries `tid`
    (pipeline.py:662-667), missing frames are filled by `bfill(limit=2)` then `ffill(limit=2)` (:678-681);
  * 2D key points of frame t: the top-down stage on that box, `zeros((K, 3))` where the box is still NaN
    (wrappers/mmpose.py:67-69);
  * 3D joints of frame t: VideoPose3D on the window [t-121, t+121] of that 2D track, edge-replicated at the two
    ends of the CLIP only (wrappers/videopose3d.py:66-75), zero rows included.

Both fills and the lifting look into the future, so the streaming form has latency: the box of an absent frame is
decided once the next two frames are known, and frame t is lifted once frame t+121 has its key points; `advance(final=
True)` (end of clip) emits the rest with the reference's edge replication.  Same FLOPs as the eager form.
The reference stores rows for ALL frames of the clip per subject; here (tid, t) pairs are emitted from the track's first
filled frame to its last one (a track the tracker has dropped is finalised at once: its future is known to be absent),
each equal to the reference's value for that frame.  One reference quirk is followed on a best-effort basis:
`process_videopose3d` normalises a float32 key-point array in float32 and a float64 one (any zero row in the clip makes
the stacked array float64) in float64; a stream uses float32 arithmetic while every frame so far had a box and float64
afterwards, which is what the reference does unless the first absent frame comes later in the clip (then earlier frames
differ by <= 1 float32 ulp of the normalised input).

The compute stages are callables, so this module needs no GPU (tests/test_person_stream.py):
    topdown_fn(jobs)  jobs = [(track_id, frame, tlwh float64[4])] -> [len(jobs)][K][3] float32
    lift_fn(kn)       kn = (n, K, 2) normalised key points -> (n, J, 3)
    lift_many_fn(kns) optional: kns = list of such contexts -> list of (n_i, J, 3), element i equal to lift_fn(kns[i]); when given,
                      advance() makes ONE call with the contexts of every stream instead of one lift_fn call per stream

`PersonStreams(lifter="GastNet")` streams the reference's DEFAULT lifting method instead (LiftingMethodLookup row 0,
wrappers/gastnet.process_gastnet), whose temporal rule is another one: GAST-Net drops the invalid frames of a track and lifts the
COMPACTED sequence of the valid ones, where VideoPose3D keeps zero rows in place.

  * Per frame: every decided 2D row (a zero row where the box stayed NaN; the first 17 joints of a wider head) goes, on its own,
    through the H36M conversion of `h36m_coco_format`, `revise_kpts` and `normalize_screen_coordinates` (rounded to float32): the
    arithmetic of process_gastnet, one frame at a time.  A frame is VALID iff its 34 converted coordinates do not sum to 0.
  * The lifted sequence is the track's valid frames only, in order; the window of the i-th valid frame is valid frames
    i - pad .. i + pad, edge-replicated at the two ends of the track's VALID sequence (so a window spans a gap of invalid frames).
  * Latency: a valid frame is lifted once `pad` further valid frames of its track are decided, or when the stream is final or
    ended (the same final / ended / cap logic as above).  With pad = 13 that is 13 valid frames, against VideoPose3D's 121 frames.
  * `keypoints_3d` rows are emitted for consecutive frames, zero rows at the invalid ones; an invalid frame waits for the valid
    frames before it.  `keypoints_valid` / `keypoints_valid_frames` ({tid: bool array} / the same frame numbers) go alongside.
  * lift_fn(x) / lift_many_fn(xs): x = (n, 17, 2) float32 consecutive VALID rows -> (n, 17, 3), each output a function of its window
    of 2 pad + 1 rows, the window edge-replicated at the two ends of x (GastNetLifter.lift_many).  A range of valid frames [a, b) is
    handed over with its context [a - pad, b + pad) cut to the valid sequence known so far; rows [a, b) of the result are kept: their
    windows lie inside the context, or end where the track's valid sequence does.  Every range that becomes computable in one
    advance() goes through ONE lift_many_fn call.
  * Declared differences to the table chain.  `h36m_coco_format` converts nothing when the coordinates of the WHOLE CLIP sum to
    exactly 0 (`kp.sum() != 0.0`); a stream never sees the whole clip and applies the per-frame rule only: the two differ only if the
    whole clip's coordinates cancel to exactly 0.  A track without any valid frame is a ValueError of process_gastnet; a stream emits
    its zero rows.  The stream converts the float32 rows of the top-down stage; a table that holds the same values as float64 (rows
    stacked with float64 zero rows) evaluates the five joints the conversion builds in float64 before rounding them to float32.
"""
from __future__ import annotations

import numpy as np

from .wrappers.videopose3d import normalize_screen_coordinates

FILL_LIMIT = 2          # PersonBbox.make: fillna(method="bfill"/"ffill", limit=2), pipeline.py:680-681


class _PersonStream:
    """Streaming PersonBbox(keep_tracks=[tid]) -> TopDownPerson -> LiftingPerson state of one track id."""

    def __init__(self, tid: int, born: int, num_joints: int):
        self.tid = tid
        self.first = max(0, born - FILL_LIMIT)   # first frame with a (back-filled) box
        self.raw: dict = {}                      # frame -> tlwh of frames whose neighbours' fills are still open
        self.last_raw = born                     # last frame with a raw (un-filled) box
        self.next_dec = self.first               # next frame whose box has not been decided
        self.k2_base = self.first                # frame index of k2[0]
        self.k2: list = []                       # decided 2D rows (K,3) float32, zeros where the box stayed NaN
        self.next3d = self.first                 # next frame whose 3D has not been emitted
        self.any_absent = self.first > 0         # reference: a zero row makes the clip's key-point array float64
        self.live = True
        self.k = num_joints
        # lifter="GastNet": the compacted sequence of valid frames
        self.g_flags: list = []                  # validity of the decided frames from next3d on (not yet emitted)
        self.g_rows: list = []                   # normalised (17,2) float32 rows of the valid frames a window can still read
        self.g_base = 0                          # index, in the valid sequence, of g_rows[0]
        self.g_next = 0                          # index, in the valid sequence, of the next valid frame to lift

    def decide(self, n_frames: int, final: bool):
        """Box decisions for frames [next_dec, n_frames) in order, as far as they can be made.  final: nothing will
        ever be added to `raw` (end of clip, or the tracker dropped the id).  Yields (frame, tlwh or None)."""
        raw = self.raw
        while self.next_dec < n_frames:
            t = self.next_dec
            box = raw.get(t)
            if box is None:
                # bfill(limit=2): the next valid row, if it is at most 2 frames ahead
                for d in range(1, FILL_LIMIT + 1):
                    if t + d in raw:
                        box = raw[t + d]
                        break
                    if t + d >= n_frames and not final:
                        return                       # frame t+d not tracked yet: undecidable for now
                if box is None:
                    # ffill(limit=2) over what is still missing: the previous valid row, at most 2 frames back
                    for d in range(1, FILL_LIMIT + 1):
                        if t - d in raw:
                            box = raw[t - d]
                            break
            self.next_dec = t + 1
            raw.pop(t - FILL_LIMIT, None)            # nothing looks further back than 2 frames
            yield t, box

    def row(self, t: int, n_total):
        """2D row of frame t for the lifting context (n_total: clip length when known, else None)."""
        if n_total is not None and t >= n_total:
            t = n_total - 1                          # np.pad(..., 'edge') at the end of the clip
        if t < 0:
            t = 0                                    # ... and at its start
        i = t - self.k2_base
        if i < 0 or i >= len(self.k2):
            return None                              # before the first box / after the track ended: a zero row
        return self.k2[i]


class PersonStreams:
    """max_persons: tracks followed at the same time (new ids are adopted, in row order, while fewer are live; an id that
    appears while max_persons others are live is never followed); keep_tracks: follow exactly these ids instead."""

    def __init__(self, num_joints: int, pad: int, src_hw, topdown_fn, lift_fn, max_persons: int = 1, keep_tracks=None,
                 lift_many_fn=None, lifter: str = "VideoPose3D"):
        if lifter not in ("VideoPose3D", "GastNet"):
            raise ValueError(f"PersonStreams: lifter = {lifter!r}, expected 'VideoPose3D' or 'GastNet'")
        if lifter == "GastNet" and int(num_joints) < 17:
            raise ValueError(f"PersonStreams: the GAST-Net rule converts the 17 COCO joints; the 2D stage has {num_joints}")
        self.lifter = lifter
        self.k, self.pad, self.src = int(num_joints), int(pad), tuple(src_hw)
        self.topdown_fn, self.lift_fn, self.lift_many_fn = topdown_fn, lift_fn, lift_many_fn
        self.max_persons = max_persons
        self.keep_tracks = None if keep_tracks is None else set(int(k) for k in keep_tracks)
        self.n_frames = 0             # frames tracked so far
        self.streams: dict = {}       # track_id -> _PersonStream (followed ids that still owe output)
        self.ignored: set = set()
        self.finished: set = set()    # followed ids whose stream was completed and emitted (their tracker said they were gone)

    def ingest(self, chunk_tracks, live_sets=None):
        """chunk_tracks: per frame, rows (track_id, x1, y1, x2, y2, score[, tlwh]) as the tracking stage reports them.  Records the
        raw presence of the followed ids (exactly one row of the frame carries the id, pipeline.py:662-667).
        live_sets: per frame, the ids the tracker can still report later (Tracker.live_ids after that frame); default: the
        ids of the frame's rows, which is the live set of both built trackers (they report every track they keep)."""
        for i, rows in enumerate(chunk_tracks):
            t = self.n_frames
            count: dict = {}
            for r in rows:
                count[r[0]] = count.get(r[0], 0) + 1
            live = count if live_sets is None else live_sets[i]
            for st in self.streams.values():
                if st.live and st.tid not in live:
                    st.live = False
            for r in rows:
                tid, x1, y1, x2, y2 = r[:5]
                if tid in self.ignored:
                    continue
                if tid in self.finished:
                    # the stream of this id was closed because the tracker's live set no longer held it; a second stream would
                    # emit frames that do not continue the first one.  Trackers that retain ids across misses must pass
                    # live_sets (SortReidTracker.live_ids / ByteTracker.live_ids do).
                    raise RuntimeError(f"track id {tid} re-appeared in frame {t} after its stream was finished: pass live_sets= "
                                       "for a tracker that keeps ids alive across missed frames")
                st = self.streams.get(tid)
                if st is None:
                    if self.keep_tracks is not None:
                        follow = tid in self.keep_tracks
                    else:
                        follow = sum(1 for s in self.streams.values() if s.live) < self.max_persons
                    if not follow:
                        self.ignored.add(tid)
                        continue
                    st = self.streams[tid] = _PersonStream(tid, t, self.k)
                if count[tid] == 1:
                    # tlhw as the wrappers store it: [x1, y1, x2 - x1, y2 - y1] on mmtrack's float32 row (wrappers/mmtrack.py:55),
                    # or the tracker's own to_tlwh() when the row carries it as a 7th element (deep_sort_yolov4/parser.py:80)
                    st.raw[t] = (np.array(r[6], np.float64) if len(r) > 6 else np.array([x1, y1, x2 - x1, y2 - y1], np.float64))
                    st.last_raw = t
            self.n_frames += 1

    def _lift_context(self, st: _PersonStream, lo: int, hi: int, n_total):
        """normalised 2D context [lo - pad, hi + pad) of one stream: what lifting frames [lo, hi) reads"""
        pad = self.pad
        zero = np.zeros((self.k, 3), np.float32)
        rows = [st.row(t, n_total) for t in range(lo - pad, hi + pad)]
        arr = np.stack([zero if r is None else r for r in rows])[:, :, :2]
        arr = arr.astype(np.float64) if st.any_absent else arr          # the reference's dtype-dependent normalisation
        return normalize_screen_coordinates(arr, self.src[1], self.src[0])

    def _lift_range(self, st: _PersonStream, lo: int, hi: int, n_total):
        """3D of frames [lo, hi) of one stream from the context [lo - pad, hi + pad)"""
        pad = self.pad
        out = self.lift_fn(self._lift_context(st, lo, hi, n_total))
        return out[pad:pad + hi - lo]

    def _gast_convert(self, st: _PersonStream, n_new: int):
        """the GAST-Net host chain on the n_new rows decided last, frame by frame: validity flags and the valid rows, normalised"""
        from .wrappers import gastnet as gw
        rows = np.stack(st.k2[len(st.k2) - n_new:])
        kpts, scores = gw.h36m_rows(rows[:, :gw.NUM_JOINTS, :2], rows[:, :gw.NUM_JOINTS, 2])
        valid = kpts.reshape(-1, 2 * gw.NUM_JOINTS).sum(axis=1) != 0
        kpts = gw.revise_kpts(kpts, scores, np.flatnonzero(valid))
        x = gw.normalize_screen_coordinates(kpts[valid], w=int(self.src[1]), h=int(self.src[0])).astype(np.float32)
        st.g_flags.extend(bool(v) for v in valid)
        st.g_rows.extend(x)

    def _gast_range(self, st: _PersonStream, bound: int, closed: bool):
        """What stream `st` can emit now, frames [next3d, next3d + m) with m > 0, or None.  bound: first frame that cannot be emitted
        yet; closed: no further valid frame will come.  -> (m, validity of the m frames, rows to keep = (offset, count) in the lifted
        context, context (n, 17, 2) or None when no frame of the range is valid); advances the stream's state."""
        pad = self.pad
        n_valid = st.g_base + len(st.g_rows)
        n_avail = min(len(st.g_flags), bound - st.next3d)
        a = b = st.g_next
        m = 0
        while m < n_avail:
            if st.g_flags[m]:
                if not closed and b + pad >= n_valid:
                    break                            # this valid frame's window is not complete: it, and what follows, waits
                b += 1
            m += 1
        if m == 0:
            return None
        mask = np.array(st.g_flags[:m], bool)
        ctx_rows, lo = None, a
        if b > a:
            lo, hi = max(0, a - pad), min(n_valid, b + pad)
            ctx_rows = np.stack(st.g_rows[lo - st.g_base:hi - st.g_base])
        del st.g_flags[:m]
        st.next3d += m
        st.g_next = b
        drop = b - pad - st.g_base                   # valid rows no window will read again
        if drop > 0:
            del st.g_rows[:drop]
            st.g_base += drop
        return m, mask, (a - lo, b - a), ctx_rows

    def advance(self, final: bool = False):
        """Decide boxes, run 2D, emit 3D for everything that has become computable.  final: end of clip.
        Returns dict(keypoints / keypoints_frames = {track_id: (n,K,3) / (n,) frame numbers} decided in this call,
                     keypoints_3d / keypoints_3d_frames = {track_id: (m,J,3) / (m,)} emitted in this call;
                     lifter="GastNet": also keypoints_valid / keypoints_valid_frames = {track_id: (m,) bool / (m,)})."""
        gast = self.lifter == "GastNet"
        kpv, gast_jobs = {}, []       # GastNet: (track_id, frames, validity, (offset, count), context) of every range emitted
        n1 = self.n_frames
        jobs, decided = [], {}
        for tid in sorted(self.streams):
            st = self.streams[tid]
            for t, box in st.decide(n1, final or not st.live):
                decided.setdefault(tid, []).append(t)
                if box is not None:
                    jobs.append((tid, t, box))
        rows2d = self.topdown_fn(jobs) if jobs else []
        k2 = {(j[0], j[1]): r for j, r in zip(jobs, rows2d)}
        kp, kp_frames, kp3, kp3_frames = {}, {}, {}, {}
        pad = self.pad
        zero = np.zeros((self.k, 3), np.float32)
        batched = []                  # lift_many_fn: (track_id, frames lifted, context) of every range that became computable
        for tid in sorted(self.streams):
            st = self.streams[tid]
            ts = decided.get(tid, [])
            for t in ts:
                row = k2.get((tid, t))
                if row is None:
                    st.any_absent = True
                    row = zero
                st.k2.append(row)
            # a dropped track owes nothing past its last (forward-filled) box: the rows after it are zero rows for good
            cap = None if st.live else st.last_raw + FILL_LIMIT + 1
            te = [t for t in ts if cap is None or t < cap]
            if te:
                kp[tid] = np.stack(st.k2[te[0] - st.k2_base: te[-1] + 1 - st.k2_base])
                kp_frames[tid] = np.array(te, np.int64)
            # ... and is finalised once its last decided row is one of those zero rows
            ended = (not st.live) and st.next_dec > cap
            if gast:
                if ts:
                    self._gast_convert(st, len(ts))
                got = self._gast_range(st, st.next_dec if cap is None else min(st.next_dec, cap), final or ended)
                if got is not None:
                    kp3_frames[tid] = np.arange(st.next3d - got[0], st.next3d, dtype=np.int64)
                    kpv[tid] = got[1]
                    gast_jobs.append((tid,) + got)
                if final or ended:
                    del self.streams[tid]
                    self.finished.add(tid)
                else:
                    del st.k2[:]                      # the compacted rows are kept instead (g_rows)
                    st.k2_base = st.next_dec
                continue
            if final:
                hi, n_total = st.next_dec if cap is None else min(st.next_dec, cap), n1
            elif ended:
                hi, n_total = cap, None
            else:
                hi, n_total = st.next_dec - pad, None
            if hi > st.next3d:
                if self.lift_many_fn is None:
                    kp3[tid] = self._lift_range(st, st.next3d, hi, n_total)
                else:                 # the context is built here, from the rows the stream holds now; lifted below, all at once
                    batched.append((tid, hi - st.next3d, self._lift_context(st, st.next3d, hi, n_total)))
                kp3_frames[tid] = np.arange(st.next3d, hi, dtype=np.int64)
                st.next3d = hi
            if final or ended:
                del self.streams[tid]
                self.finished.add(tid)
            else:
                drop = st.next3d - pad - st.k2_base       # rows no window will read again
                if drop > 0:
                    del st.k2[:drop]
                    st.k2_base += drop
        if batched:
            lifted = self.lift_many_fn([kn for _, _, kn in batched])
            assert len(lifted) == len(batched), (len(lifted), len(batched))
            for (tid, n, _), out in zip(batched, lifted):
                kp3[tid] = out[pad:pad + n]
        if gast:
            todo = [j for j in gast_jobs if j[4] is not None]
            if todo and self.lift_many_fn is not None:
                lifted = self.lift_many_fn([j[4] for j in todo])
                assert len(lifted) == len(todo), (len(lifted), len(todo))
            else:
                lifted = [self.lift_fn(j[4]) for j in todo]
            lifted = {j[0]: out for j, out in zip(todo, lifted)}
            for tid, m, mask, (off, cnt), _ in gast_jobs:
                out3 = np.zeros((m, 17, 3), np.float32)
                if cnt:
                    out3[mask] = np.asarray(lifted[tid])[off:off + cnt]
                kp3[tid] = out3
            return dict(keypoints=kp, keypoints_frames=kp_frames, keypoints_3d=kp3, keypoints_3d_frames=kp3_frames,
                        keypoints_valid=kpv, keypoints_valid_frames={tid: f.copy() for tid, f in kp3_frames.items()})
        return dict(keypoints=kp, keypoints_frames=kp_frames, keypoints_3d=kp3, keypoints_3d_frames=kp3_frames)


def collect(outs, what="keypoints_3d"):
    """Stitch advance() / Cascade.step() results: {track_id: (first_frame, array over consecutive frames)}."""
    acc: dict = {}
    for o in outs:
        for tid, arr in o[what].items():
            fr_ = o[what + "_frames"][tid]
            a = acc.setdefault(tid, ([], []))
            a[0].append(np.asarray(fr_))
            a[1].append(np.asarray(arr))
    res = {}
    for tid, (f, a) in acc.items():
        f, a = np.concatenate(f), np.concatenate(a)
        assert np.array_equal(f, np.arange(f[0], f[0] + len(f))), (tid, f)       # consecutive, in order, once each
        res[tid] = (int(f[0]), a)
    return res
