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

Structure: `_PersonStream` holds what does not depend on the lifter (the box decisions of one track id); a lifter's temporal rule is
a subclass that owns its rows (`_FrameWindows`: VideoPose3D, `_ValidWindows`: GAST-Net; `push` takes the new 2D rows, `emit` says
which frames can be emitted now, what has to be lifted for them and where the lifted rows go).  `PersonStreams.advance` is one path
for both: decide boxes, run the 2D stage, hand every stream its rows, collect the contexts the streams hand back, lift them in one
call (or one after the other, in ascending track-id order), place the results.

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
    """Streaming PersonBbox(keep_tracks=[tid]) -> TopDownPerson -> LiftingPerson state of one track id: the box decisions, which do
    not depend on the lifter.  A lifter's temporal rule is a subclass with its own state and two methods:

        push(rows, absent)            the 2D rows (K,3) decided last, consecutive frames (zero rows where the box stayed NaN; absent:
                                      there is one among them)
        emit(bound, closed, n_total)  bound: first frame that cannot be emitted yet; closed: no further row will come; n_total: the
                                      clip's length once it is known, else None.  -> None, or (m, context, place, more) and next3d moved
                                      on by m > 0: frames [next3d - m, next3d) are emitted now; context: what to lift for them, or None
                                      when nothing is; place(lifted context, or None) -> their (m, J, 3) block; more: {name: (m,) per-
                                      frame values} for the names in `extra`.  Also forgets the rows no later window will read."""

    extra = ()                                   # names of what the rule emits per frame beside keypoints_3d

    def __init__(self, tid: int, born: int, num_joints: int, pad: int, src_hw):
        self.tid = tid
        self.first = max(0, born - FILL_LIMIT)   # first frame with a (back-filled) box
        self.raw: dict = {}                      # frame -> tlwh of frames whose neighbours' fills are still open
        self.last_raw = born                     # last frame with a raw (un-filled) box
        self.next_dec = self.first               # next frame whose box has not been decided
        self.next3d = self.first                 # next frame whose 3D has not been emitted
        self.live = True
        self.k, self.pad, self.src = num_joints, pad, src_hw

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


class _FrameWindows(_PersonStream):
    """VideoPose3D's rule: zero rows stay in place, the window of frame t is the frames [t - pad, t + pad] of the clip."""

    def __init__(self, *args):
        super().__init__(*args)
        self.k2_base = self.first                # frame index of k2[0]
        self.k2: list = []                       # decided 2D rows (K,3) float32, zeros where the box stayed NaN
        self.any_absent = self.first > 0         # reference: a zero row makes the clip's key-point array float64

    def push(self, rows, absent: bool):
        self.any_absent = self.any_absent or absent
        self.k2.extend(rows)

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

    def emit(self, bound: int, closed: bool, n_total):
        pad, lo = self.pad, self.next3d
        hi = bound if closed else bound - pad        # frame t waits for the key points of frame t + pad
        got = None
        if hi > lo:
            # normalised 2D context [lo - pad, hi + pad): what lifting frames [lo, hi) reads
            zero = np.zeros((self.k, 3), np.float32)
            rows = [self.row(t, n_total) for t in range(lo - pad, hi + pad)]
            arr = np.stack([zero if r is None else r for r in rows])[:, :, :2]
            arr = arr.astype(np.float64) if self.any_absent else arr          # the reference's dtype-dependent normalisation
            got = (hi - lo, normalize_screen_coordinates(arr, self.src[1], self.src[0]), lambda out: out[pad:pad + hi - lo], {})
            self.next3d = hi
        drop = self.next3d - pad - self.k2_base       # rows no window will read again
        if drop > 0:
            del self.k2[:drop]
            self.k2_base += drop
        return got


class _ValidWindows(_PersonStream):
    """GAST-Net's rule: the invalid frames are dropped, the window of the i-th VALID frame is valid frames [i - pad, i + pad]."""

    extra = ("keypoints_valid",)

    def __init__(self, *args):
        super().__init__(*args)
        self.flags: list = []                    # validity of the decided frames from next3d on (not yet emitted)
        self.rows: list = []                     # normalised (17,2) float32 rows of the valid frames a window can still read
        self.base = 0                            # index, in the valid sequence, of rows[0]
        self.next_valid = 0                      # index, in the valid sequence, of the next valid frame to lift

    def push(self, rows, absent: bool):
        """the GAST-Net host chain on the new rows, frame by frame: validity flags and the valid rows, normalised"""
        if not rows:
            return
        from .wrappers import gastnet as gw
        rows = np.stack(rows)
        kpts, scores = gw.h36m_rows(rows[:, :gw.NUM_JOINTS, :2], rows[:, :gw.NUM_JOINTS, 2])
        valid = kpts.reshape(-1, 2 * gw.NUM_JOINTS).sum(axis=1) != 0
        kpts = gw.revise_kpts(kpts, scores, np.flatnonzero(valid))
        x = gw.normalize_screen_coordinates(kpts[valid], w=int(self.src[1]), h=int(self.src[0])).astype(np.float32)
        self.flags.extend(bool(v) for v in valid)
        self.rows.extend(x)

    def emit(self, bound: int, closed: bool, n_total):
        pad = self.pad
        n_valid = self.base + len(self.rows)
        n_avail = min(len(self.flags), bound - self.next3d)
        a = b = self.next_valid
        m = 0
        while m < n_avail:
            if self.flags[m]:
                if not closed and b + pad >= n_valid:
                    break                            # this valid frame's window is not complete: it, and what follows, waits
                b += 1
            m += 1
        if m == 0:
            return None
        mask = np.array(self.flags[:m], bool)
        ctx_rows, lo = None, a
        if b > a:                                    # the context [a - pad, b + pad) cut to the valid sequence known so far
            lo, hi = max(0, a - pad), min(n_valid, b + pad)
            ctx_rows = np.stack(self.rows[lo - self.base:hi - self.base])
        del self.flags[:m]
        self.next3d += m
        self.next_valid = b
        drop = b - pad - self.base                   # valid rows no window will read again
        if drop > 0:
            del self.rows[:drop]
            self.base += drop

        def place(out):
            out3 = np.zeros((m, 17, 3), np.float32)      # zero rows at the invalid frames
            if b > a:
                out3[mask] = np.asarray(out)[a - lo:b - lo]
            return out3
        return m, ctx_rows, place, {"keypoints_valid": mask}


_RULES = {"VideoPose3D": _FrameWindows, "GastNet": _ValidWindows}       # PersonStreams(lifter=...)


class PersonStreams:
    """max_persons: tracks followed at the same time (new ids are adopted, in row order, while fewer are live; an id that
    appears while max_persons others are live is never followed); keep_tracks: follow exactly these ids instead."""

    def __init__(self, num_joints: int, pad: int, src_hw, topdown_fn, lift_fn, max_persons: int = 1, keep_tracks=None,
                 lift_many_fn=None, lifter: str = "VideoPose3D"):
        if lifter not in _RULES:
            raise ValueError(f"PersonStreams: lifter = {lifter!r}, expected 'VideoPose3D' or 'GastNet'")
        if lifter == "GastNet" and int(num_joints) < 17:
            raise ValueError(f"PersonStreams: the GAST-Net rule converts the 17 COCO joints; the 2D stage has {num_joints}")
        self.lifter, self._rule = lifter, _RULES[lifter]
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
                    st = self.streams[tid] = self._rule(tid, t, self.k, self.pad, self.src)
                if count[tid] == 1:
                    # tlhw as the wrappers store it: [x1, y1, x2 - x1, y2 - y1] on mmtrack's float32 row (wrappers/mmtrack.py:55),
                    # or the tracker's own to_tlwh() when the row carries it as a 7th element (deep_sort_yolov4/parser.py:80)
                    st.raw[t] = (np.array(r[6], np.float64) if len(r) > 6 else np.array([x1, y1, x2 - x1, y2 - y1], np.float64))
                    st.last_raw = t
            self.n_frames += 1

    def advance(self, final: bool = False):
        """Decide boxes, run 2D, emit 3D for everything that has become computable.  final: end of clip.
        Returns dict(keypoints / keypoints_frames = {track_id: (n,K,3) / (n,) frame numbers} decided in this call,
                     keypoints_3d / keypoints_3d_frames = {track_id: (m,J,3) / (m,)} emitted in this call;
                     lifter="GastNet": also keypoints_valid / keypoints_valid_frames = {track_id: (m,) bool / (m,)})."""
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
        more = {name: {} for name in self._rule.extra}
        zero = np.zeros((self.k, 3), np.float32)
        emitted = []                  # (track_id, context or None, place) of every range emitted, in ascending track-id order
        for tid in sorted(self.streams):
            st = self.streams[tid]
            ts = decided.get(tid, [])
            new = [k2.get((tid, t)) for t in ts]
            rows = [zero if r is None else r for r in new]
            st.push(rows, any(r is None for r in new))
            # a dropped track owes nothing past its last (forward-filled) box: the rows after it are zero rows for good
            cap = None if st.live else st.last_raw + FILL_LIMIT + 1
            te = [t for t in ts if cap is None or t < cap]
            if te:
                kp[tid] = np.stack(rows[:len(te)])
                kp_frames[tid] = np.array(te, np.int64)
            # ... and is finalised once its last decided row is one of those zero rows
            ended = (not st.live) and st.next_dec > cap
            got = st.emit(st.next_dec if cap is None else min(st.next_dec, cap), final or ended, n1 if final else None)
            if got is not None:
                m, context, place, vals = got
                kp3_frames[tid] = np.arange(st.next3d - m, st.next3d, dtype=np.int64)
                for name in more:
                    more[name][tid] = vals[name]
                emitted.append((tid, context, place))
            if final or ended:
                del self.streams[tid]
                self.finished.add(tid)
        # the contexts are built above, from the rows the streams held then; lifted here, all at once
        contexts = [c for _, c, _ in emitted if c is not None]
        if contexts and self.lift_many_fn is not None:
            lifted = self.lift_many_fn(contexts)
            assert len(lifted) == len(contexts), (len(lifted), len(contexts))
        else:
            lifted = [self.lift_fn(c) for c in contexts]
        lifted = iter(lifted)
        for tid, context, place in emitted:
            kp3[tid] = place(None if context is None else next(lifted))
        out = dict(keypoints=kp, keypoints_frames=kp_frames, keypoints_3d=kp3, keypoints_3d_frames=kp3_frames)
        for name, vals in more.items():
            out[name] = vals
            out[name + "_frames"] = {tid: kp3_frames[tid].copy() for tid in vals}
        return out


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
