"""Hot-path tables of PosePipe with the reference's names, `definition` strings and `make()` dispatch.

Mirrors pose_pipeline/pipeline.py for exactly the tables the detect/track -> 2D -> 3D cascade touches
(file:line of each table next to its class).  The other 38 tables of the reference
are sibling method branches / rendering and are out of scope.  Backed by posepipeline_amd.djshim unless
POSEPIPE_USE_DATAJOINT=1 selects the real DataJoint package (then `definition` strings create the same
MySQL schema as the reference).

Videos: the reference stores an `attach@localattach` and re-decodes it with OpenCV in every stage
(`Video.get_robust_reader`, pipeline.py:47-87).  Here `video` holds a path; posepipeline_amd.video
reads it (OpenCV when importable, otherwise the raw `.npy`/`.ppvid` containers used by tests and bench).
"""
from __future__ import annotations

import os

import numpy as np

if os.environ.get("POSEPIPE_USE_DATAJOINT") == "1":  # the real package (MySQL); tests/test_entry_script.py runs this branch on a stand-in
    import datajoint as dj
else:
    from . import djshim as dj

from . import video as _video

if "custom" not in dj.config:
    dj.config["custom"] = {}
db_prefix = dj.config["custom"].get("database.prefix", "")
schema = dj.schema(db_prefix + "pose_pipeline")


@schema
class Video(dj.Manual):  # pipeline.py:25-33
    definition = """
    # Table containing raw videos, grouped by project and filename, with their start time
    video_project       : varchar(50)
    filename            : varchar(100)
    ---
    video               : attach@localattach    # datajoint managed video file
    start_time          : timestamp(3)          # time of beginning of video, as accurately as known
    import_time  = CURRENT_TIMESTAMP : timestamp
    """

    @staticmethod
    def get_robust_reader(key, return_cap=True):
        """pipeline.py:47-87: the path of a readable copy of the video (or an opened reader): every announced frame must
        decode, else the file is transcoded with the reference's ffmpeg command and read from the transcode
        (video.robust_path; validated once per file instead of once per stage).  Unlike the reference the attachment is not
        moved into a temporary file: `video` holds a path the caller owns, and the wrappers do not delete it."""
        path = _video.robust_path((Video & key).fetch1("video"))
        if return_cap:
            return _video.open_video(path)
        return path


@schema
class VideoInfo(dj.Computed):  # pipeline.py:92-102
    definition = """
    # Video info including timestamps, delta times, num frames, height and width
    -> Video
    ---
    timestamps      : longblob
    delta_time      : longblob
    fps             : float
    height          : int
    width           : int
    num_frames      : int
    """

    def make(self, key, override=False):
        from datetime import timedelta
        key = key.copy()
        path, start_time = (Video & key).fetch1("video", "start_time")
        src = _video.open_video(path)
        fps = float(src.fps)
        if fps < 1:
            raise Exception("FPS is less than 1")
        key["fps"] = fps
        key["num_frames"] = frames = int(src.num_frames)
        key["width"], key["height"] = int(src.width), int(src.height)
        key["timestamps"] = [start_time + timedelta(0, i / fps) for i in range(frames)]
        key["delta_time"] = [timedelta(0, i / fps).total_seconds() for i in range(frames)]
        src.release()
        self.insert1(key)


@schema
class BottomUpMethodLookup(dj.Lookup):  # pipeline.py:133-147
    definition = """
    bottom_up_method_name : varchar(50)
    """
    contents = [
        {"bottom_up_method_name": "OpenPose"},
        {"bottom_up_method_name": "OpenPose_BODY25B"},
        {"bottom_up_method_name": "OpenPose_HR"},
        {"bottom_up_method_name": "OpenPose_LR"},
        {"bottom_up_method_name": "MMPose"},
        # this uses the COCO25 keypoints but in the same order as OpenPose
        {"bottom_up_method_name": "Bridging_OpenPose"},
    ]


@schema
class BottomUpMethod(dj.Manual):  # pipeline.py:150-155
    definition = """
    -> Video
    -> BottomUpMethodLookup
    """


@schema
class BottomUpPeople(dj.Computed):  # pipeline.py:158-165
    definition = """
    -> BottomUpMethod
    ---
    keypoints                   : longblob
    timestamp=CURRENT_TIMESTAMP : timestamp    # automatic timestamp
    """

    def make(self, key):  # pipeline.py:167-245
        if key["bottom_up_method_name"] == "MMPose":
            from .wrappers.mmpose import mmpose_bottom_up
            key["keypoints"] = mmpose_bottom_up(key)
        else:          # the OpenPose / Bridging rows need third-party code that is not built
            raise Exception("Method not implemented")
        self.insert1(key)


@schema
class TrackingBboxMethodLookup(dj.Lookup):  # pipeline.py:480-494
    definition = """
    tracking_method      : int
    ---
    tracking_method_name : varchar(50)
    """
    contents = [
        {"tracking_method": 0, "tracking_method_name": "DeepSortYOLOv4"},
        {"tracking_method": 1, "tracking_method_name": "MMTrack_tracktor"},
        {"tracking_method": 2, "tracking_method_name": "FairMOT"},
        {"tracking_method": 3, "tracking_method_name": "TransTrack"},
        {"tracking_method": 4, "tracking_method_name": "TraDeS"},
        {"tracking_method": 5, "tracking_method_name": "MMTrack_deepsort"},
        {"tracking_method": 6, "tracking_method_name": "MMTrack_bytetrack"},
        {"tracking_method": 7, "tracking_method_name": "MMTrack_qdtrack"},
    ]


@schema
class TrackingBboxMethod(dj.Manual):  # pipeline.py:499-503
    definition = """
    -> Video
    tracking_method   : int
    ---
    """


@schema
class TrackingBbox(dj.Computed):  # pipeline.py:508-513
    definition = """
    -> TrackingBboxMethod
    ---
    tracks            : longblob
    num_tracks        : int
    """

    def make(self, key):  # pipeline.py:515-578
        video = Video.get_robust_reader(key, return_cap=False)
        name = (TrackingBboxMethodLookup & key).fetch1("tracking_method_name")
        if name == "DeepSortYOLOv4":       # pipeline.py:519-523
            from .wrappers.deep_sort_yolov4.parser import tracking_bounding_boxes
            tracks = tracking_bounding_boxes(video)
        elif name in "MMTrack_tracktor":   # sic: substring test, pipeline.py:525
            from .wrappers.mmtrack import mmtrack_bounding_boxes
            tracks = mmtrack_bounding_boxes(video, "tracktor")
        elif name == "MMTrack_deepsort":
            from .wrappers.mmtrack import mmtrack_bounding_boxes
            tracks = mmtrack_bounding_boxes(video, "deepsort")
        elif name == "MMTrack_bytetrack":
            from .wrappers.mmtrack import mmtrack_bounding_boxes
            tracks = mmtrack_bounding_boxes(video, "bytetrack")
        elif name == "MMTrack_qdtrack":
            from .wrappers.mmtrack import mmtrack_bounding_boxes
            tracks = mmtrack_bounding_boxes(video, "qdtrack")
        elif name == "FairMOT":            # pipeline.py:549-553
            from .wrappers.fairmot import fairmot_bounding_boxes
            tracks = fairmot_bounding_boxes(video)
        elif name == "TraDeS":             # pipeline.py:561-565
            from .wrappers.trades import trades_bounding_boxes
            tracks = trades_bounding_boxes(video)
        else:
            raise Exception(f"Unsupported tracking method: {key['tracking_method']}")
        key["tracks"] = tracks
        track_ids = np.unique([t["track_id"] for track in tracks for t in track])
        key["num_tracks"] = len(track_ids)
        self.insert1(key)


@schema
class PersonBboxValid(dj.Manual):  # pipeline.py:639-644
    definition = """
    -> TrackingBbox
    video_subject_id        : int
    ---
    keep_tracks             : longblob
    """


@schema
class PersonBbox(dj.Computed):  # pipeline.py:649-654
    definition = """
    -> PersonBboxValid
    ---
    bbox               : longblob
    present            : longblob
    """

    def make(self, key):  # pipeline.py:656-687
        from .tracking import person_bbox
        tracks = (TrackingBbox & key).fetch1("tracks")
        keep_tracks = (PersonBboxValid & key).fetch1("keep_tracks")
        key["bbox"], key["present"] = person_bbox(tracks, keep_tracks)
        self.insert1(key)

    @property
    def key_source(self):  # pipeline.py:705-707
        return PersonBboxValid & "video_subject_id >= 0"


@schema
class DetectedFrames(dj.Computed):  # pipeline.py:712-722
    definition = """
    -> PersonBboxValid
    -> VideoInfo
    ---
    frames_detected        : int
    frames_missed          : int
    fraction_found         : float
    mean_other_people      : float
    median_confidence      : float
    frame_data             : longblob
    """

    def make(self, key):  # pipeline.py:724-762
        tracks = (TrackingBbox & key).fetch1("tracks")
        keep_tracks = (PersonBboxValid & key).fetch1("keep_tracks")
        stats = []
        for fr in tracks:
            valid = [t for t in fr if t["track_id"] in keep_tracks]
            if len(valid) == 1:
                stats.append({"present": True, "confidence": valid[0].get("confidence", 1.0), "others": len(fr) - 1})
            else:
                stats.append({"present": False, "confidence": 0, "others": len(fr)})
        present = np.array([s["present"] for s in stats])
        key["frames_detected"] = np.sum(present)
        key["frames_missed"] = np.sum(~present)
        key["fraction_found"] = key["frames_detected"] / (key["frames_missed"] + key["frames_detected"])
        key["median_confidence"] = (np.median([s["confidence"] for s in stats if s["present"]])
                                    if key["frames_detected"] > 0 else 0.0)
        key["mean_other_people"] = np.nanmean([s["others"] for s in stats])
        key["frame_data"] = stats
        self.insert1(key)

    @property
    def key_source(self):
        return PersonBboxValid & "video_subject_id >= 0"


@schema
class BestDetectedFrames(dj.Computed):  # pipeline.py:770-785
    definition = """
    -> DetectedFrames
    """

    def make(self, key):  # pipeline.py:775-781: of a video's DetectedFrames rows, the one whose subject is found most often
        rows = (DetectedFrames & key).fetch("fraction_found", "KEY", as_dict=True)
        best = dict(rows[int(np.argmax([r["fraction_found"] for r in rows]))])
        best.pop("fraction_found")
        self.insert1(best)

    @property
    def key_source(self):  # pipeline.py:783-785
        return Video & DetectedFrames


@schema
class BottomUpPerson(dj.Computed):  # pipeline.py:788-795
    definition = """
    -> PersonBbox
    -> BottomUpPeople
    ---
    keypoints        : longblob
    """

    def make(self, key):  # pipeline.py:797-810
        from .keypoint_matching import match_keypoints_to_bbox
        print(key)
        keypoints = (BottomUpPeople & key).fetch1("keypoints")
        bbox = (PersonBbox & key).fetch1("bbox")
        # num_keypoints=17: the reference leaves the default 25 (OpenPose), so an unmatched frame of a COCO track is a (25, 3)
        # row among (17, 3) rows and `np.array` gives a ragged object array; 17 keeps the result rectangular
        res = [match_keypoints_to_bbox(bbox[idx], keypoints[idx], num_keypoints=17) for idx in range(bbox.shape[0])]
        keypoints, _ = list(zip(*res))
        key["keypoints"] = np.array(keypoints)
        self.insert1(key)


@schema
class TopDownMethodLookup(dj.Lookup):  # pipeline.py:979-998
    definition = """
    top_down_method      : int
    ---
    top_down_method_name : varchar(50)
    """
    contents = [
        {"top_down_method": 0, "top_down_method_name": "MMPose"},
        {"top_down_method": 1, "top_down_method_name": "MMPoseWholebody"},
        {"top_down_method": 2, "top_down_method_name": "MMPoseHalpe"},
        {"top_down_method": 3, "top_down_method_name": "MMPoseHrformerCoco"},
        {"top_down_method": 4, "top_down_method_name": "OpenPose"},
        {"top_down_method": 6, "top_down_method_name": "OpenPose_BODY25B"},
        {"top_down_method": 7, "top_down_method_name": "MMPoseTCFormerWholebody"},
        {"top_down_method": 8, "top_down_method_name": "OpenPose_HR"},
        {"top_down_method": 9, "top_down_method_name": "OpenPose_LR"},
        {"top_down_method": 11, "top_down_method_name": "Bridging_COCO_25"},
        {"top_down_method": 12, "top_down_method_name": "Bridging_bml_movi_87"},
        {"top_down_method": 13, "top_down_method_name": "Bridging_smpl+head_30"},
        {"top_down_method": 14, "top_down_method_name": "Bridging_smplx_42"},
        # NOT a row of the reference (ViTPose is absent from it): BASELINE.json configs[4], ids above the reference's range
        {"top_down_method": 100, "top_down_method_name": "ViTPoseB"},
        {"top_down_method": 101, "top_down_method_name": "ViTPoseL"},
        {"top_down_method": 102, "top_down_method_name": "ViTPoseH"},
    ]


@schema
class TopDownMethod(dj.Manual):  # pipeline.py:1003-1006
    definition = """
    -> PersonBbox
    top_down_method    : int
    """


@schema
class TopDownPerson(dj.Computed):  # pipeline.py:1011-1015
    definition = """
    -> TopDownMethod
    ---
    keypoints          : longblob
    """

    def make(self, key):  # pipeline.py:1017-1095
        method_name = (TopDownMethodLookup & key).fetch1("top_down_method_name")
        from .wrappers.mmpose import mmpose_top_down_person
        if method_name == "MMPose":
            key["keypoints"] = mmpose_top_down_person(key, "HRNet_W48_COCO")
        elif method_name == "MMPoseWholebody":
            key["keypoints"] = mmpose_top_down_person(key, "HRNet_W48_COCOWholeBody")
        elif method_name == "MMPoseHalpe":
            key["keypoints"] = mmpose_top_down_person(key, "HRNet_W48_HALPE")
        elif method_name == "MMPoseHrformerCoco":
            key["keypoints"] = mmpose_top_down_person(key, "HRFormer_COCO")
        elif method_name in ("ViTPoseB", "ViTPoseL", "ViTPoseH"):      # extension, see TopDownMethodLookup
            key["keypoints"] = mmpose_top_down_person(key, "ViTPose_%s_COCO" % method_name[-1])
        else:
            raise Exception("Method not implemented")
        self.insert1(key)

    @staticmethod
    def joint_names(method="MMPose"):
        from .wrappers.mmpose import mmpose_joint_dictionary
        return mmpose_joint_dictionary[method]


@schema
class SkeletonAction(dj.Computed):  # pipeline.py:1145-1156
    definition = """
    -> TopDownPerson
    method            : varchar(50)
    ---
    top5              : longblob
    action_scores     : longblob
    label_map         : longblob
    action_window_len : int
    stride            : int
    computed_timestamp=CURRENT_TIMESTAMP : timestamp    # automatic timestamp
    """

    def make(self, key):  # pipeline.py:1160-1166
        from .wrappers.mmaction import mmaction_skeleton_action_person

        key = mmaction_skeleton_action_person(key, stride=1)
        key["method"] = "mmaction_skeleton"
        self.insert1(key)


@schema
class LiftingMethodLookup(dj.Lookup):  # pipeline.py:1226-1239
    definition = """
    lifting_method      : int
    ---
    lifting_method_name : varchar(50)
    """
    contents = [
        {"lifting_method": 0, "lifting_method_name": "GastNet"},
        {"lifting_method": 1, "lifting_method_name": "VideoPose3D"},
        {"lifting_method": 2, "lifting_method_name": "PoseAug"},
        {"lifting_method": 11, "lifting_method_name": "Bridging_COCO_25"},
        {"lifting_method": 12, "lifting_method_name": "Bridging_bml_movi_87"},
        {"lifting_method": 13, "lifting_method_name": "Bridging_smpl+head_30"},
        {"lifting_method": 14, "lifting_method_name": "Bridging_smplx_42"},
    ]


@schema
class LiftingMethod(dj.Manual):  # pipeline.py:1244-1247
    definition = """
    -> TopDownPerson
    -> LiftingMethodLookup
    """


@schema
class LiftingPerson(dj.Computed):  # pipeline.py:1252-1257
    definition = """
    -> LiftingMethod
    ---
    keypoints_3d       : longblob
    keypoints_valid    : longblob
    """

    def make(self, key):  # pipeline.py:1259-1416
        name = (LiftingMethodLookup & key).fetch1("lifting_method_name")
        if name == "VideoPose3D":
            from .wrappers.videopose3d import process_videopose3d
            results = process_videopose3d(key)
        elif name == "GastNet":  # pipeline.py:1265-1269; as there, only where the model is installed (the reference: GAST_PATH)
            from .wrappers import gastnet
            if not os.path.exists(gastnet.checkpoint_path()):
                raise Exception(f"Method not implemented {key}: the GAST-Net checkpoint {gastnet.checkpoint_path()} is not installed")
            results = gastnet.process_gastnet(key)
        else:
            raise Exception(f"Method not implemented {key}")
        key.update(results)
        self.insert1(key)

    @staticmethod
    def joint_names():
        """Lifting layers use Human3.6 ordering (pipeline.py:1418-1438)"""
        return ["Hip (root)", "Right hip", "Right knee", "Right foot", "Left hip", "Left knee", "Left foot", "Spine",
                "Thorax", "Nose", "Head", "Left shoulder", "Left elbow", "Left wrist", "Right shoulder", "Right elbow",
                "Right wrist"]


# ---- SMPL stage (pipeline.py:1513-1640) ----------------------------------------------------------------------------------
@schema
class SMPLMethodLookup(dj.Lookup):  # pipeline.py:1515-1530
    definition = """
    smpl_method       : int
    ---
    smpl_method_name  : varchar(50)
    """
    contents = [
        {"smpl_method": 0, "smpl_method_name": "VIBE"},
        {"smpl_method": 1, "smpl_method_name": "MEVA"},
        {"smpl_method": 2, "smpl_method_name": "ProHMR"},
        {"smpl_method": 3, "smpl_method_name": "Expose"},
        {"smpl_method": 4, "smpl_method_name": "PARE"},
        {"smpl_method": 5, "smpl_method_name": "PIXIE"},
        {"smpl_method": 6, "smpl_method_name": "ProHMR_MMPose"},
        {"smpl_method": 7, "smpl_method_name": "HybrIK"},
    ]


@schema
class SMPLMethod(dj.Manual):  # pipeline.py:1534-1538
    definition = """
    -> PersonBbox
    -> SMPLMethodLookup
    """


@schema
class SMPLPerson(dj.Computed):  # pipeline.py:1542-1552
    definition = """
    -> SMPLMethod
    ---
    model_type      : varchar(50)
    cams            : longblob
    poses           : longblob
    betas           : longblob
    joints3d        : longblob
    joints2d        : longblob
    """

    def make(self, key):  # pipeline.py:1556-1620
        name = (SMPLMethodLookup & key).fetch1("smpl_method_name")
        if name == "VIBE":
            from .wrappers.vibe import process_vibe
            res = process_vibe(key)
            res["model_type"] = "SMPL"
        else:                                   # MEVA, ProHMR, Expose, PARE, PIXIE, ProHMR_MMPose, HybrIK: not built
            raise Exception(f"Method {name} not implemented")
        res.pop("verts", None)                  # :1617-1618: the mesh is computed but not stored
        self.insert1(res)

    @staticmethod
    def joint_names(model="smpl"):  # pipeline.py:1622-1631
        if model.upper() == "SMPL":
            from .models.smpl import JOINT_NAMES_49
            return list(JOINT_NAMES_49)
        raise NotImplementedError(f"joint names of model {model!r}: only the SMPL methods' 49 joints are built")


# ---- hand stage (pipeline.py:1979-2146) --------------------------------------------------------------------------------
@schema
class HandBboxMethodLookup(dj.Lookup):  # pipeline.py:1980-1990
    definition = """
    detection_method      : int
    ---
    detection_method_name : varchar(50)
    """
    contents = [
        {"detection_method": 0, "detection_method_name": "RTMDet"},
        {"detection_method": 1, "detection_method_name": "TopDown"},
    ]


@schema
class HandBboxMethod(dj.Manual):  # pipeline.py:1993-1998
    definition = """
    -> Video
    -> HandBboxMethodLookup
    ---
    """


@schema
class HandBbox(dj.Computed):  # pipeline.py:2002-2008
    definition = """
    -> HandBboxMethod
    ---
    num_boxes   :   int
    bboxes      :   longblob
    """

    def make(self, key):  # pipeline.py:2009-2029
        name = (HandBboxMethodLookup & key).fetch1("detection_method_name")
        if name == "RTMDet":
            from .wrappers.hand_bbox import mmpose_hand_det
            num_boxes, bboxes = mmpose_hand_det(key=key, method="RTMDet")      # not built: raises NotImplementedError
            key["bboxes"] = bboxes
            key["num_boxes"] = num_boxes
        elif name == "TopDown":
            # right / left hand boxes from the Halpe keypoints of the TopDownPerson table
            from .wrappers.hand_bbox import make_bbox_from_keypoints
            try:
                keypoints = (TopDownPerson & key & "top_down_method=2").fetch1("keypoints")
            except Exception:
                raise Exception("TopDownPerson table does not have the required keypoints")
            key["bboxes"] = make_bbox_from_keypoints(keypoints)
            key["num_boxes"] = 2
        else:
            raise Exception("Method not implemented")
        self.insert1(key)


_HAND_JOINTS = ["Wrist", "CMC1", "MCP1", "IP1", "TIP1", "MCP2", "PIP2", "DIP2", "TIP2", "MCP3", "PIP3", "DIP3", "TIP3", "MCP4",
                "PIP4", "DIP4", "TIP4", "MCP5", "PIP5", "DIP5", "TIP5"]
_HAND_JOINTS_RHD = ["Wrist", "TIP1", "IP1", "MCP1", "CMC1", "TIP2", "DIP2", "PIP2", "MCP2", "TIP3", "DIP3", "PIP3", "MCP3", "TIP4",
                    "DIP4", "PIP4", "MCP4", "TIP5", "DIP5", "PIP5", "MCP5"]


@schema
class HandPoseEstimationMethodLookup(dj.Lookup):  # pipeline.py:2032-2045
    definition = """
    estimation_method      : int
    ---
    estimation_method_name : varchar(50)
    """
    contents = [
        {"estimation_method": -1, "estimation_method_name": "Halpe"},
        {"estimation_method": 0, "estimation_method_name": "RTMPoseHand5"},
        {"estimation_method": 1, "estimation_method_name": "RTMPoseCOCO"},
        {"estimation_method": 2, "estimation_method_name": "freihand"},
        {"estimation_method": 3, "estimation_method_name": "HRNet_dark"},
        {"estimation_method": 4, "estimation_method_name": "HRNet_udp"},
    ]

    def joint_names(self):
        """pipeline.py:2047-2103, called on a restricted view: `(HandPoseEstimationMethodLookup & key).joint_names()`.  42 names
        (right, then left) for every method but HRNet_dark, whose 21 names are the rhd2d joint order (the reference's quirk)."""
        method = self.fetch1("estimation_method_name")
        if method in ("RTMPoseHand5", "RTMPoseCOCO", "freihand", "HRNet_udp", "Halpe"):
            return [n.lower() + "_r" for n in _HAND_JOINTS] + [n.lower() + "_l" for n in _HAND_JOINTS]
        elif method == "HRNet_dark":
            return list(_HAND_JOINTS_RHD)


@schema
class HandPoseEstimationMethod(dj.Manual):  # pipeline.py:2107-2112
    definition = """
    -> HandBbox
    -> HandPoseEstimationMethodLookup
    ---
    """


@schema
class HandPoseEstimation(dj.Computed):  # pipeline.py:2116-2121
    definition = """
    -> HandPoseEstimationMethod
    ---
    keypoints_2d       : longblob  #(time, [21 righthand-21 lefthand], 3)
    """

    def make(self, key):  # pipeline.py:2122-2146
        name = (HandPoseEstimationMethodLookup & key).fetch1("estimation_method_name")
        if name in ("HRNet_dark", "HRNet_udp"):
            from .wrappers.hand_estimation import mmpose_HPE
            key["keypoints_2d"] = mmpose_HPE(key, name)
        elif name == "Halpe":      # the hands of the Halpe-136 body model themselves: right 21, then left 21
            kp2d = (TopDownPerson & key & "top_down_method=2").fetch1("keypoints")
            key["keypoints_2d"] = np.concatenate((kp2d[:, -21:, :], kp2d[:, -42:-21, :]), axis=1)
        else:                      # RTMPoseHand5 / RTMPoseCOCO / freihand: other model families, not built
            raise Exception("Method not implemented")
        self.insert1(key)
