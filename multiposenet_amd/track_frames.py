"""Persons with persistent identities over the frames of a video.

    python -m multiposenet_amd.track_frames --images DIR --out tracks.jsonl
        [--model keypoints.npz] [--detector detector.npz] [--prn prn.npz] [--dtype bf16|f32] [--size W H] [--batch 16]
        [--similarity oks|iou] [--assignment greedy|optimal] [--match-threshold 0.3] [--max-misses 10] [--new-track-score 0.3] [--max-tracks 32]
        [--score-threshold 0.05] [--smooth [--fps 30] [--min-cutoff 1.0] [--beta 0.007] [--d-cutoff 1.0]
        [--min-keypoint-score 0.0]]
        [--motion [--velocity-gain 0.5] [--damping 1.0]]
        [--pose-nms [THRESHOLD]] [--pose-nms-min-keypoint-score X] [--pose-nms-score box|box*keypoints]
        [--frames-out DIR [--jpeg-quality 75] [--label-size 10] [--draw-smoothed] [--hide-untracked]]
        [--anonymize [head|box] [--anonymize-mode pixelate|blur|fill] [--anonymize-shape ellipse|rectangle] [--anonymize-blocks 8]
        [--anonymize-radius 8] [--anonymize-no-overlay]]
        [--crops-out DIR [--crop-size H W] [--crop-pad P] [--crop-fit stretch|pad] [--crop-quality Q]]
        [--annotations JSON [--eval-threshold 0.5]]
        [--zones FILE.json]
        [--trails [LENGTH] [--trail-every N] [--trail-max-gap N] [--trail-anchor feet|box_bottom|box_centre] [--no-trail-fade]
        [--no-trail-draw]]
        [--density [CELL] [--density-footprint anchor|box] [--density-half-life N] [--density-show dwell|visits]
        [--density-full-scale N] [--density-opacity A] [--no-density-smooth] [--no-density-draw] [--density-out FILE.npz]]

The image files of DIR, in sorted name order, are the frames of ONE stream. They go through the Detector in batches of
--batch consecutive frames with `track=` a `tracking.PoseTracker`: the matching runs inside the captured graph and the track
state stays on the device between the batches. JPEG files go through `Detector.predict_jpegs` as the bytes they are (every
route `jpeg.jpeg_support` names); a batch holding any other file is decoded by Pillow and goes through `predict_images`.
The last, shorter batch runs at its own size (a second graph of that size): padding it with copies of the last frame would
advance the tracks by frames the video does not have. --out gets one JSON line per frame: its name, and per person the
track id (0 = untracked), the box (ymin, xmin, ymax, xmax, normalised to the frame) and the keypoints (x, y, score) in the
frame's pixels. --smooth runs a One-Euro filter over every tracked joint on the device as well (`tracking.OneEuro`; --fps is
the video's frame rate) and adds "keypoints_smoothed" (x, y, score) and "keypoint_velocities" (pixels per second) to every
line; beta multiplies a speed in frame pixels and so depends on the resolution. --motion matches every frame's persons
against where the tracks are expected (`tracking.ConstantVelocity`: a velocity per track, --velocity-gain the weight of a new
observation of it, --damping its decay per frame without a detection) and adds "coasting_ids", "coasting_boxes" and
"coasting_keypoints" (x, y) to every line: the tracks that are alive but were not detected in the frame, at their predicted
pose. --pose-nms drops duplicate poses in front of the tracker (`pose_nms=`, an `inference.PoseNms`: keypoint-similarity NMS
inside the same graph; alone it uses the class's default threshold, which is not tuned). --frames-out DIR also writes every frame as
DIR/<name>.jpg with its persons drawn on it - box, keypoints and an id label in a colour per track (`inference.TrackStyle`;
--draw-smoothed draws the smoothed keypoints, --hide-untracked leaves persons without an id out) - drawn and JPEG-encoded on
the device in the same graph ('annotated_jpeg'); the JSON lines are the same with and without it. --anonymize (with
--frames-out) makes every detected person unrecognisable in those frames first (`anonymize=`, an `inference.Anonymize`: one more
stage in the same graph; the head by default, or the whole box; --anonymize-no-overlay writes the anonymised frames without
boxes, skeletons and ids; the class's defaults are not tuned). --crops-out DIR writes the picture of every detected person as
DIR/<frame name>_<k>.jpg, or DIR/<frame name>_id<track id>.jpg when the person has an id (`crops=`, an `inference.PersonCrops`
with format='jpeg': cut, resized and JPEG-encoded on the device in the same graph; the bytes are written as they arrive, not
encoded again on the host; with --anonymize the crops show the anonymised frames). --annotations JSON (a
COCO-style file whose annotations carry `track_id`, PoseTrack's layout; frames are found by the base name of `file_name`, a frame
the file does not name has no annotated person) scores the identities while it tracks (`track_eval=`, a
`track_metrics.TrackEvaluator`: one more launch in the same graph; a pair can correspond at OKS >= --eval-threshold) and adds
MOTA, MOTP, IDF1 and the counts behind them to the summary as "track_eval". --zones FILE.json counts the tracked persons in
polygons and across lines while it tracks (`zones=`, a `zones.ZoneCounter`: one more launch in the same graph). The file holds
"frame_size" [height, width], named "zones" {name: [[x, y], ...]} and "lines" {name: [[x, y], [x, y]]} in the frames' pixels and,
optionally, "anchor", "min_frames" and "min_keypoint_score". Every line gains "zones": per person the names of the zones it is
inside ("inside") and its events ("entered", "exited", "crossed_positive", "crossed_negative"), and for the frame "occupancy",
"entries", "exits", "line_positive" and "line_negative" by name; the summary gains the totals by name as "zones". A frame of
another size than frame_size ends the run with a ValueError. --trails [LENGTH] keeps the last LENGTH anchors of every tracked
person on the device while it tracks (`trails=`, a `trails.TrackTrails`: one more launch in the same graph; alone it uses the
class's default length, which is not tuned; the frames' size is that of the first frame, and a frame of another size ends the run
with a ValueError). Every line gains "trail": per person its points (x, y), newest first, empty for a person without an id.
With --frames-out the trails are drawn into the written frames in the persons' colours (`mpn_draw_trails`, two more launches),
fading towards their old end unless --no-trail-fade; --no-trail-draw keeps them out of the frames. --trail-every N keeps one
point per N frames, --trail-max-gap N starts a new trail for a person not seen for more than N frames (0: never). --density [CELL] accumulates where the persons stand over a grid of CELL x CELL pixel cells on the device while
it tracks (`density=`, a `density.DensityMap`: one more launch in the same graph; alone it uses the class's default cell, which is
not tuned; the frames' size is that of the first frame, and a frame of another size ends the run with a ValueError). Every line
gains "density": per person its "cell" (row, col; -1, -1 outside the frame) and the frame's "counted", "visits", "max_dwell" and
"max_visits". With --frames-out the map is laid over the written frames (`mpn_draw_density`, two more launches) unless
--no-density-draw: --density-show says which plane, --density-full-scale N the count at which the colour saturates (0: each
frame's own maximum), --density-opacity A the alpha of the highest level, --no-density-smooth draws whole cells.
--density-footprint box adds a person to every cell whose centre its box covers, --density-half-life N halves every counter
once per N frames (0: never). --density-out FILE.npz writes the final "dwell" and "visits" planes and "cell". Without model files the weights are seeded random ones: the output then only shows that the path runs."""
import argparse
import json
import os

import numpy as np

EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp")


def _is_jpeg(data):
    from .inference.jpeg import jpeg_support
    try:
        jpeg_support(data)
    except ValueError:
        return False
    return True


def _pixels(data):
    import io

    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", required=True, help="directory of frames; sorted by name")
    ap.add_argument("--out", default="tracks.jsonl")
    ap.add_argument("--model", help="keypoint model .npz (the shared backbone)")
    ap.add_argument("--detector", help="person detector head .npz")
    ap.add_argument("--prn", help="pose residual network .npz")
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--size", type=int, nargs=2, default=(640, 640), metavar=("W", "H"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--similarity", choices=("oks", "iou"), default="oks")
    ap.add_argument("--assignment", choices=("greedy", "optimal"), default="greedy",
                    help="how a frame's persons are matched to the tracks: the largest similarity first, or the optimal assignment")
    ap.add_argument("--match-threshold", type=float, default=0.3)
    ap.add_argument("--max-misses", type=int, default=10)
    ap.add_argument("--new-track-score", type=float, default=0.3)
    ap.add_argument("--max-tracks", type=int, default=32)
    ap.add_argument("--score-threshold", type=float, default=0.05)
    ap.add_argument("--smooth", action="store_true", help="One-Euro smoothing of the tracked keypoints, and their velocities")
    ap.add_argument("--fps", type=float, default=30.0, help="frame rate of the video (--smooth)")
    ap.add_argument("--min-cutoff", type=float, default=1.0)
    ap.add_argument("--beta", type=float, default=0.007)
    ap.add_argument("--d-cutoff", type=float, default=1.0)
    ap.add_argument("--min-keypoint-score", type=float, default=0.0)
    ap.add_argument("--motion", action="store_true",
                    help="match against the tracks' constant-velocity prediction and report the coasting tracks")
    ap.add_argument("--velocity-gain", type=float, default=0.5, help="weight of a newly observed velocity, 0..1 (--motion)")
    ap.add_argument("--damping", type=float, default=1.0, help="factor on a track's velocity per frame without a detection, 0..1 (--motion)")
    ap.add_argument("--frames-out", metavar="DIR", help="write every frame as DIR/<name>.jpg with its tracked persons drawn on it")
    ap.add_argument("--jpeg-quality", type=int, default=75, help="of the written frames (--frames-out)")
    ap.add_argument("--label-size", type=int, default=10, help="font size of the id labels (--frames-out)")
    ap.add_argument("--draw-smoothed", action="store_true", help="draw the smoothed keypoints (--frames-out, needs --smooth)")
    ap.add_argument("--hide-untracked", action="store_true", help="leave persons without an id out of the frames (--frames-out)")
    ap.add_argument("--annotations", metavar="JSON", help="PoseTrack-style annotations: evaluate the tracks (MOTA, IDF1) while tracking")
    ap.add_argument("--eval-threshold", type=float, default=0.5, help="OKS at which a person can correspond to an annotation (--annotations)")
    ap.add_argument("--zones", metavar="FILE.json",
                    help="count the tracked persons in polygons and across lines: frame_size, named zones and lines, "
                         "optionally anchor, min_frames, min_keypoint_score")
    ap.add_argument("--trails", metavar="LENGTH", type=int, nargs="?", const=-1, default=None,
                    help="keep the last LENGTH anchors of every tracked person (alone: the class's default) and write them as \"trail\"")
    ap.add_argument("--trail-every", metavar="N", type=int, default=None, help="keep one point per N frames (--trails)")
    ap.add_argument("--trail-max-gap", metavar="N", type=int, default=None,
                    help="a person not seen for more than N frames starts a new trail; 0: never (--trails)")
    ap.add_argument("--trail-anchor", choices=("feet", "box_bottom", "box_centre"), default=None,
                    help="the point that stands for a person (--trails)")
    ap.add_argument("--no-trail-fade", action="store_true", help="draw every segment of a trail opaque (--trails, --frames-out)")
    ap.add_argument("--no-trail-draw", action="store_true", help="keep the trails out of the written frames (--trails, --frames-out)")
    ap.add_argument("--density", metavar="CELL", type=int, nargs="?", const=-1, default=None,
                    help="accumulate where the persons stand over cells of CELL x CELL pixels (alone: the class's default) and "
                         "write each person's cell as \"density\"")
    ap.add_argument("--density-footprint", choices=("anchor", "box"), default=None,
                    help="a person adds to its anchor's cell, or to every cell whose centre its box covers (--density)")
    ap.add_argument("--density-half-life", metavar="N", type=int, default=None,
                    help="halve every counter once per N frames; 0: never (--density)")
    ap.add_argument("--density-show", choices=("dwell", "visits"), default=None, help="the plane the frames show (--density)")
    ap.add_argument("--density-full-scale", metavar="N", type=int, default=None,
                    help="the count at which the colour saturates; 0: each frame's own maximum (--density, --frames-out)")
    ap.add_argument("--density-opacity", metavar="A", type=int, default=None,
                    help="the alpha of the highest level, 0..255 (--density, --frames-out)")
    ap.add_argument("--no-density-smooth", action="store_true", help="draw whole cells (--density, --frames-out)")
    ap.add_argument("--no-density-draw", action="store_true", help="keep the map out of the written frames (--density, --frames-out)")
    ap.add_argument("--density-out", metavar="FILE.npz", default=None,
                    help="write the final dwell and visits planes and the cell size (--density)")
    from . import pose_nms
    from .inference import anonymize_stage
    from .inference import crops as crops_stage
    pose_nms.add_arguments(ap)
    anonymize_stage.add_arguments(ap)
    crops_stage.add_arguments(ap)
    args = ap.parse_args(argv)
    if args.batch < 1:
        ap.error("--batch must be at least 1")
    nms = pose_nms.from_arguments(ap, args)
    anon = anonymize_stage.from_arguments(ap, args)
    if anon is not None and args.frames_out is None:
        ap.error("--anonymize changes the frames --frames-out writes: it needs --frames-out DIR")
    trail_options = None
    if args.trails is None:
        if args.trail_every is not None or args.trail_max_gap is not None or args.trail_anchor is not None or args.no_trail_fade \
                or args.no_trail_draw:
            ap.error("--trail-every, --trail-max-gap, --trail-anchor, --no-trail-fade and --no-trail-draw need --trails")
    else:
        trail_options = dict(fade=not args.no_trail_fade, draw=not args.no_trail_draw, min_keypoint_score=args.min_keypoint_score)
        for key, value in (("length", None if args.trails == -1 else args.trails), ("every", args.trail_every), ("max_gap", args.trail_max_gap),
                           ("anchor", args.trail_anchor)):
            if value is not None:
                trail_options[key] = value
    density_options = None
    if args.density is None:
        if args.density_footprint is not None or args.density_half_life is not None or args.density_show is not None or \
                args.density_full_scale is not None or args.density_opacity is not None or args.no_density_smooth or \
                args.no_density_draw or args.density_out is not None:
            ap.error("--density-footprint, --density-half-life, --density-show, --density-full-scale, --density-opacity, "
                     "--no-density-smooth, --no-density-draw and --density-out need --density")
    else:
        density_options = dict(smooth=not args.no_density_smooth, draw=not args.no_density_draw,
                               min_keypoint_score=args.min_keypoint_score)
        for key, value in (("cell", None if args.density == -1 else args.density), ("footprint", args.density_footprint),
                           ("half_life", args.density_half_life), ("show", args.density_show), ("full_scale", args.density_full_scale),
                           ("opacity", args.density_opacity)):
            if value is not None:
                density_options[key] = value
    motion = None
    if args.motion:
        from .tracking import ConstantVelocity
        try:
            motion = ConstantVelocity(velocity_gain=args.velocity_gain, damping=args.damping)
        except ValueError as e:
            ap.error(str(e))
    names = sorted(f for f in os.listdir(args.images) if f.lower().endswith(EXTENSIONS))
    if not names:
        raise SystemExit(f"no image files {EXTENSIONS} under {args.images}")

    import torch
    from .evaluate_pose import _random_head
    from .inference import Detector, OneEuro, PoseTracker, TrackStyle
    from .prn import initial_values
    smooth = None
    if args.smooth:
        try:
            smooth = OneEuro(rate=args.fps, min_cutoff=args.min_cutoff, beta=args.beta, d_cutoff=args.d_cutoff,
                             min_keypoint_score=args.min_keypoint_score)
        except ValueError as e:
            ap.error(str(e))
    draw = {}
    if args.frames_out is not None:
        if args.draw_smoothed and smooth is None:
            ap.error("--draw-smoothed needs --smooth")
        try:
            style = TrackStyle(label_size=args.label_size, keypoints="smoothed" if args.draw_smoothed else "frame",
                               untracked="hide" if args.hide_untracked else "plain")
            style.tables()
        except ValueError as e:
            ap.error(str(e))
        draw = dict(annotate="jpeg", jpeg_quality=args.jpeg_quality, track_style=style)
        if anon is not None:
            draw["anonymize"] = anon
            if not anon.overlay:
                draw["track_style"] = None                          # nothing is drawn over the anonymised frames
        os.makedirs(args.frames_out, exist_ok=True)
    if args.detector is None or args.prn is None:
        print("[track_frames] no --detector / --prn file: seeded random weights, the tracks mean nothing")
    det = Detector(args.model, dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32,
                   detector_path=args.detector if args.detector is not None else _random_head(),
                   prn_path=args.prn if args.prn is not None else initial_values(seed=0))
    tracker = PoseTracker(streams=1, max_tracks=args.max_tracks, similarity=args.similarity, match_threshold=args.match_threshold,
                          max_misses=args.max_misses, new_track_score=args.new_track_score, max_boxes=det.params['max_boxes'],
                          smooth=smooth, motion=motion, assignment=args.assignment)
    size = (args.size[1], args.size[0])
    evaluator, annotated = None, {}
    if args.annotations is not None:
        from .track_metrics import TrackEvaluator, groundtruth_from_posetrack
        annotated = {os.path.basename(name): gt for name, gt in groundtruth_from_posetrack(args.annotations)}
        evaluator = TrackEvaluator(streams=1, threshold=args.eval_threshold, max_boxes=det.params['max_boxes'])
    counter = None
    if args.zones is not None:
        from .zones import ZoneCounter
        with open(args.zones) as f:
            spec = json.load(f)
        unknown = sorted(set(spec) - {"frame_size", "zones", "lines", "anchor", "min_frames", "min_keypoint_score"})
        if unknown or "frame_size" not in spec:
            ap.error(f"--zones: {args.zones} must hold frame_size, zones and / or lines, and optionally anchor, min_frames, "
                     f"min_keypoint_score (unknown: {unknown})")
        try:
            counter = ZoneCounter(streams=1, max_boxes=det.params['max_boxes'], **spec)
        except ValueError as e:
            ap.error(str(e))
    cut = crops_stage.from_arguments(ap, args, det.params['max_boxes'])
    if cut is not None:
        os.makedirs(args.crops_out, exist_ok=True)
    trails = density = None
    nobody = {'keypoints': np.zeros((0, 17, 3)), 'boxes': np.zeros((0, 4)), 'track_ids': np.zeros(0, np.int64)}
    frames = persons = 0
    with open(args.out, "w") as out:
        for at in range(0, len(names), args.batch):
            batch = names[at:at + args.batch]
            files = []
            for name in batch:
                with open(os.path.join(args.images, name), "rb") as f:
                    files.append(f.read())
            scored = {}
            if evaluator is not None:
                scored = dict(groundtruth=[annotated.get(name, nobody) for name in batch], track_eval=evaluator)
            if counter is not None:
                scored["zones"] = counter
            if (trail_options is not None and trails is None) or (density_options is not None and density is None):
                if _is_jpeg(files[0]):                              # the first frame says in whose pixels trails and map are
                    from .inference.jpeg import jpeg_info
                    info = jpeg_info(files[0])
                    first_size = (info['height'], info['width'])
                else:
                    first_size = _pixels(files[0]).shape[:2]
            if density_options is not None and density is None:
                from .density import DensityMap
                try:
                    density = DensityMap(streams=1, frame_size=tuple(int(v) for v in first_size), max_boxes=det.params['max_boxes'],
                                         **density_options)
                except ValueError as e:
                    ap.error(str(e))
            if density is not None:
                scored["density"] = density
            if trail_options is not None and trails is None:
                from .trails import TrackTrails
                try:
                    trails = TrackTrails(streams=1, frame_size=first_size, max_boxes=det.params['max_boxes'], **trail_options)
                except ValueError as e:
                    ap.error(str(e))
            if trails is not None:
                scored["trails"] = trails
            if cut is not None:
                scored["crops"] = cut
            if all(_is_jpeg(data) for data in files):
                outs = det.predict_jpegs(files, size=size, score_threshold=args.score_threshold, track=tracker, pose_nms=nms,
                                        **draw, **scored)
            else:
                outs = det.predict_images([_pixels(data) for data in files], size=size, score_threshold=args.score_threshold,
                                          track=tracker, pose_nms=nms, **draw, **scored)
            if evaluator is not None:
                evaluator.collect(outs)
            for name, o in zip(batch, outs):
                line = {"name": name, "ids": o["track_ids"].tolist(), "boxes": o["boxes"].tolist(),
                        "keypoints": o["keypoints"].tolist()}
                if smooth is not None:
                    line["keypoints_smoothed"] = o["keypoints_smoothed"].tolist()
                    line["keypoint_velocities"] = o["keypoint_velocities"].tolist()
                if motion is not None:
                    line["coasting_ids"] = o["coasting_ids"].tolist()
                    line["coasting_boxes"] = o["coasting_boxes"].tolist()
                    line["coasting_keypoints"] = o["coasting_keypoints"].tolist()
                if counter is not None:
                    z = o["zones"]
                    line["zones"] = {k: [[name for name, hit in zip(names_of, row) if hit] for row in z[k]]
                                     for k, names_of in (("inside", counter.zone_names), ("entered", counter.zone_names),
                                                         ("exited", counter.zone_names), ("crossed_positive", counter.line_names),
                                                         ("crossed_negative", counter.line_names))}
                    line["zones"].update({k: dict(zip(names_of, z[k].tolist()))
                                          for k, names_of in (("occupancy", counter.zone_names), ("entries", counter.zone_names),
                                                              ("exits", counter.zone_names), ("line_positive", counter.line_names),
                                                              ("line_negative", counter.line_names))})
                if trails is not None:
                    t = o["trails"]
                    line["trail"] = [pts[:n].tolist() if tracked else []
                                     for pts, n, tracked in zip(t["points"], t["count"], t["tracked"])]
                if density is not None:
                    d = o["density"]
                    line["density"] = {"cell": d["cell"].tolist(), "counted": d["counted"], "visits": d["visits"],
                                       "max_dwell": d["max_dwell"], "max_visits": d["max_visits"]}
                out.write(json.dumps(line) + "\n")
                if draw:
                    with open(os.path.join(args.frames_out, os.path.splitext(name)[0] + ".jpg"), "wb") as f:
                        f.write(o["annotated_jpeg"])
                if cut is not None:                                 # the device's bytes, as they are
                    for file_name, data in zip(crops_stage.crop_file_names(name, o["track_ids"], len(o["crops"])), o["crops"]):
                        with open(os.path.join(args.crops_out, file_name), "wb") as f:
                            f.write(data)
                persons += len(o["track_ids"])
            frames += len(batch)
    state = tracker.tracks(0)
    summary = {"frames": frames, "persons": persons, "ids_given": state["next_id"] - 1, "live_tracks": len(state["ids"]),
               "dropped": state["dropped"], "similarity": args.similarity, "assignment": args.assignment, "out": args.out}
    if smooth is not None:
        summary["smooth"] = {"fps": smooth.rate, "min_cutoff": smooth.min_cutoff, "beta": smooth.beta, "d_cutoff": smooth.d_cutoff,
                             "min_keypoint_score": smooth.min_keypoint_score}
    if motion is not None:
        summary["motion"] = {"velocity_gain": motion.velocity_gain, "damping": motion.damping}
    if nms is not None:
        summary["pose_nms"] = {"threshold": nms.threshold, "min_keypoint_score": nms.min_keypoint_score, "score": nms.score}
    if evaluator is not None:
        summary["track_eval"] = dict(evaluator.evaluate(), threshold=evaluator.threshold, annotations=args.annotations)
    if counter is not None:
        summary["zones"] = dict(counter.totals(0), file=args.zones)
    if trails is not None:
        summary["trails"] = {"length": trails.length, "every": trails.every, "max_gap": trails.max_gap, "anchor": trails.anchor,
                             "fade": trails.fade, "draw": trails.draw}
    if density is not None:
        summary["density"] = {"cell": density.cell, "grid": [density.gh, density.gw], "footprint": density.footprint,
                              "half_life": density.half_life, "show": density.show, "draw": density.draw,
                              "max_dwell": int(density.state(0)["max_dwell"]), "max_visits": int(density.state(0)["max_visits"])}
        if args.density_out is not None:
            np.savez(args.density_out, dwell=density.grid(0, "dwell"), visits=density.grid(0, "visits"), cell=np.int32(density.cell))
            summary["density"]["out"] = args.density_out
    print(json.dumps(summary))
    return state


if __name__ == "__main__":
    main()
