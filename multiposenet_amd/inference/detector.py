"""Detector with the reference's surface (inference/detector.py:5-61) over the JOINT inference graph of create_pb.py:44-153:

    uint8 image -> /255 -> ONE MobileNet pass -> keypoint subnet (sigmoid heatmaps, segmentation mask)
                                              -> RetinaNet head -> NMS (score 0.3, IoU 0.6, 25 boxes: create_pb.py:31-36)
                -> per-channel min-max normalised heatmaps -> crop_and_resize of every box -> PRN -> softmax / argmax_2d

and returns the seven outputs of OUTPUT_NAMES (create_pb.py:22-26) with the score filter of inference/detector.py:54-59.
The reference freezes three checkpoints into one `.pb` (create_pb.py:170-185); here the three variable sets are three `.npz`
files keyed by the reference's variable names (multiposenet_amd.checkpoint)."""
import collections
import importlib

import numpy as np
import torch

from .. import _lib
from .. import pose_metrics
from .. import pose_nms as pose_nms_stage
from ..net import KeypointNet
from . import anonymize_stage
from . import crops as crops_stage
from . import draw, jpeg, maps, resample, tta
from .record import NUM_KEYPOINTS, _ROW, RecordLayout, _no_persons, unpack_record  # noqa: F401 (found here by tests and tools)

record_layout = RecordLayout            # the layout's earlier name, when it was a tuple of slices: modules that import it still load

# create_pb.py:31-36: the thresholds frozen into the graph
PARAMS = {'depth_multiplier': 1.0, 'score_threshold': 0.3, 'iou_threshold': 0.6, 'max_boxes': 25}


def _load(path):
    """A variable set: the path of an `.npz`, or a dict of arrays already in memory."""
    if isinstance(path, dict):
        return path
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def check_batch(images):
    """The argument checks of `Detector.predict_batch`, before any device work: (b, height, width) of a uint8 [b, h, w, 3]
    array or a list of b equally sized uint8 [h, w, 3] arrays; the errors of `Detector.__call__` for a bad size or dtype."""
    if isinstance(images, np.ndarray):
        if images.ndim != 4:
            raise ValueError("images must be an array [b, height, width, 3] or a list of [height, width, 3] arrays")
        items = [images]
        b, shape = images.shape[0], tuple(images.shape[1:])
    else:
        items = list(images)
        if any(not isinstance(im, np.ndarray) for im in items):
            raise ValueError("images must be numpy arrays")
        shapes = {tuple(im.shape) for im in items}
        if len(shapes) > 1:
            raise ValueError(f"the images of a batch must have one size (got {sorted(shapes)})")
        b, shape = len(items), (shapes.pop() if shapes else ())
    if b < 1:
        raise ValueError("empty batch")
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"an image must be [height, width, 3] (got {shape})")
    h, w, _ = shape
    assert h % 128 == 0 and w % 128 == 0                          # inference/detector.py:45
    if any(im.dtype != np.uint8 for im in items):
        raise ValueError("image must be uint8")
    return b, h, w


def check_annotate(annotate, jpeg_quality, jpeg_subsampling):
    """The `annotate` argument of the predict_* methods: False or True -> None; 'jpeg' -> (quality, subsampling), checked."""
    if not isinstance(annotate, str):
        return None
    if annotate != 'jpeg':
        raise ValueError(f"annotate must be False, True or 'jpeg' (got {annotate!r})")
    jpeg.quality_tables(jpeg_quality)
    jpeg._sampling(jpeg_subsampling)
    return int(jpeg_quality), jpeg_subsampling


def check_track_style(track_style, annotate, track):
    """The `track_style` argument of the predict_* methods -> () or the tail of the entry's key. Before any device work."""
    if track_style is None:
        return ()
    if not isinstance(track_style, draw.TrackStyle):
        raise ValueError(f"track_style must be None or an inference.TrackStyle (got {track_style!r})")
    if not annotate:
        raise ValueError("track_style= says how annotate draws tracked persons: it needs annotate=True or 'jpeg'")
    if track is None:
        raise ValueError("track_style= colours persons by their track ids: it needs track=, a tracking.PoseTracker")
    if track_style.keypoints == 'smoothed' and getattr(track, 'smooth', None) is None:
        raise ValueError("track_style: keypoints='smoothed' draws the tracker's smoothed keypoints; this tracker was made "
                         "without smooth=")
    return ('style', track_style)


def check_plot_maps(plot_maps, heatmap_outputs):
    """The `plot_maps` argument of the predict_* methods -> bool. True needs a graph with heatmap outputs (a bool, or a
    callable asked only then): without them there is nothing to plot, and that is an error up front, not an empty picture."""
    if not isinstance(plot_maps, (bool, np.bool_)):
        raise ValueError(f"plot_maps must be False or True (got {plot_maps!r})")
    if plot_maps and not (heatmap_outputs() if callable(heatmap_outputs) else heatmap_outputs):
        raise ValueError("plot_maps=True needs the keypoint subnet's heatmap outputs; this Detector has none")
    return bool(plot_maps)


def check_tta(flip, scales, height, width):
    """The `flip` and `scales` arguments of the predict_* methods for a height x width network input -> the tail of the
    entry's key: () for a plain call, else ('tta', flip, ((W_k, H_k), ...)). scales: at most tta.MAX_SCALES further network
    input sizes (width, height), multiples of 128 with the base's aspect ratio, each once and none the base itself."""
    if not isinstance(flip, (bool, np.bool_)):
        raise ValueError(f"flip must be False or True (got {flip!r})")
    sizes = []
    for s in (() if scales is None else scales):
        try:
            wk, hk = (int(v) for v in s)
        except (TypeError, ValueError):
            raise ValueError(f"a scale must be (width, height) (got {s!r})")
        if wk < 128 or hk < 128 or wk % 128 or hk % 128:
            raise ValueError(f"a scale must be positive multiples of 128 (got {wk} x {hk})")
        if wk * height != hk * width:
            raise ValueError(f"scale {wk} x {hk} has another aspect ratio than the {width} x {height} base")
        if (wk, hk) == (width, height):
            raise ValueError(f"scale {wk} x {hk} is the base size itself")
        if (wk, hk) in sizes:
            raise ValueError(f"scale {wk} x {hk} is given twice")
        sizes.append((wk, hk))
    if len(sizes) > tta.MAX_SCALES:
        raise ValueError(f"at most {tta.MAX_SCALES} extra scales are merged in one launch (got {len(sizes)})")
    if not flip and not sizes:
        return ()
    return ('tta', bool(flip), tuple(sizes))


def _encode_plan(sizes, src_offsets, jp):
    """The encode of the annotated frames where mpn_draw_detections writes them (RGBA, draw.layout's offsets)."""
    _, frames, _ = draw.layout(sizes, src_offsets)
    return jpeg.EncodePlan([(h, w) for _, h, w in frames], [at for at, _, _ in frames], 4, *jp)


def _batch_frames(b, h, w):
    """(sizes, byte offsets) of the b frames of a fixed uint8 [b, h, w, 3] batch, as draw.layout and _encode_plan take them."""
    return [(h, w)] * b, [i * h * w * 3 for i in range(b)]


# The stages that write rows behind the record, in the order of their parts in the `RecordLayout` - which is also the order
# in which `_finish` unpacks them and the call commits them. part: the name of the part and of the _Entry attribute; option:
# the _Options field, and the word in an entry's key; result: the key of the result dicts the unpacked rows go to (None: they
# update the dict); tail: how the option is spelled behind its word in the key - by its 'serial', as the 'value' itself, or
# None where `_Options.tail` spells it out; stateful: the caller's own object with a prev / next state: the entry holds it
# as it is and the call commits it. The launches, which take different arguments, are written out in `_device_side_batch`.
_Stage = collections.namedtuple('_Stage', 'part option result tail stateful')
_STAGES = (_Stage('oks', 'oks', 'oks', None, False),
           _Stage('track', 'track', None, None, True),
           _Stage('nms', 'pose_nms', None, 'value', False),
           _Stage('track_eval', 'track_eval', 'track_eval', 'serial', True),
           _Stage('zones', 'zones', 'zones', 'serial', True),
           _Stage('trails', 'trails', 'trails', 'serial', True),
           _Stage('density', 'density', 'density', 'serial', True))


# The stages that ride on the tracker, by keyword: (module, class, what the messages call the stage, why it needs track= - None:
# it does not, `Detector._check_density` has the rule)
_RIDERS = {'track_eval': ('track_metrics', 'TrackEvaluator', 'the evaluator', "scores the tracker's identities"),
           'zones': ('zones', 'ZoneCounter', 'the counter', "counts the tracker's identities"),
           'trails': ('trails', 'TrackTrails', 'the trails', "follows the tracker's identities"),
           'density': ('density', 'DensityMap', 'the map', None)}


class _Options(collections.namedtuple('_Options', 'thr annotate plot_maps oks tta track style return_heatmaps track_eval crops density trails zones anonymize pose_nms')):
    """The checked options of one predict_* call (`Detector._options`): the float score threshold; annotate as False, True or
    'jpeg''s (quality, sampling); plot_maps; oks, tta and style as the parts of the key that `_check_groundtruth`, `check_tta`
    and `check_track_style` return, () where the option is off; return_heatmaps; every other field the object of its keyword,
    or None."""
    __slots__ = ()

    @property
    def jpeg(self):
        """(quality, sampling) of annotate='jpeg', else None."""
        return self.annotate if isinstance(self.annotate, tuple) else None

    def tail(self, b):
        """What the options add behind the base of an entry's key for b images: every combination an entry of its own."""
        key = ()
        if self.annotate:
            key += ('annotate', 'jpeg', self.jpeg[1]) if self.jpeg else ('annotate',)
        if self.plot_maps:
            key += ('maps',)
        key += self.oks + self.tta
        if self.track is not None:
            key += ('track', self.track.serial, b)
        key += self.style
        for st in _STAGES:
            stage = getattr(self, st.option)
            if st.tail is not None and stage is not None:
                key += (st.option, stage.serial if st.tail == 'serial' else stage)
        if self.anonymize is not None:
            key += ('anonymize', self.anonymize)
        if self.crops is not None:
            key += ('crops', self.crops)
        return key


class _Entry:
    """The persistent state behind one key of `Detector._graphs` / `_eager_batches`; what a path does not use stays None.
    stage, x: the pinned input staging and the device input. host: the pinned result buffers by output name. graph, outs, ver:
    the captured graph, its outputs and the variable versions it last ran with. draw, encode, encode_plan, maps, tta,
    anonymize: the buffers of annotate, plot_maps, flip / scales and anonymize= (draw.Buffers, jpeg.JpegBatchEncoder,
    maps.MapPlotter, tta.Buffers, anonymize_stage.Anonymizer). crops: the buffers of crops= (crops.CropBuffers). style: (TrackStyle, its table on the device). The parts of
    `_STAGES`: oks and nms are buffers of the entry (pose_metrics.OksBuffers, pose_nms.PoseNmsBuffers); track, track_eval,
    zones, trails and density are the caller's objects, whose state the graph reads and writes: the entry keeps them alive.
    layout: the RecordLayout of those parts. sources, meta_stage, meta, work, jpeg: the packed sources, descriptors (with
    their staging), intermediates and JPEG decoder of the ragged paths."""
    __slots__ = ('stage', 'x', 'host', 'graph', 'outs', 'ver', 'draw', 'encode', 'encode_plan', 'maps', 'sources', 'meta_stage',
                 'meta', 'work', 'jpeg', 'tta', 'style', 'anonymize', 'crops', 'layout') + tuple(st.part for st in _STAGES)

    def __init__(self, **buffers):
        for name in self.__slots__:
            setattr(self, name, None)
        self.host = {}
        for name, buffer in buffers.items():
            setattr(self, name, buffer)

    def commit(self):
        """The stateful stages advance their state: ONCE per call, outside the graph (`Detector._run` may launch twice)."""
        for st in _STAGES:
            if st.stateful and getattr(self, st.part) is not None:
                getattr(self, st.part).commit()


class Detector:
    def __init__(self, model_path, gpu_memory_fraction=0.25, visible_device_list='0', dtype=torch.bfloat16, prn_path=None,
                 max_boxes=None, detector_path=None, params=None):
        """
        Arguments:
            model_path: the keypoint model (create_pb.py KEYPOINTS_CHECKPOINT): `.npz`, keys = the reference's variable names,
                HWIO kernels - what `KeypointNet.state_dict()` saves / a TF checkpoint exported by tools/tf_checkpoint_to_npz.py;
                None = seeded random weights. (The reference loads ONE frozen .pb, inference/detector.py:13-19.) Its
                `MobilenetV1/*` variables are the shared backbone (create_pb.py:170-173).
            detector_path: the person detector's head (PERSON_DETECTOR_CHECKPOINT, variables `fpn/*`, `p{l}_batch_norm/*`,
                `class_net/*`, `box_net/*`; its own `MobilenetV1/*` copy, if any, is ignored like create_pb.py:178-181 maps
                only the head scope): `.npz`, a dict of arrays, or None = no boxes are detected (keypoint outputs only).
            prn_path: the pose residual network (PRN_CHECKPOINT, `PRN/fc{1,2}/{weights,biases}`): `.npz` or None.
            gpu_memory_fraction: accepted for signature compatibility, unused (buffers are sized per input shape).
            visible_device_list: a string, the GPU index.
            params: overrides of create_pb.py's PARAMS (score_threshold, iou_threshold, max_boxes).
        """
        device = f"cuda:{int(str(visible_device_list).split(',')[0])}"
        self.params = dict(PARAMS, **(params or {}))
        if max_boxes is not None:
            self.params['max_boxes'] = int(max_boxes)
        values = _load(model_path) if model_path is not None else None
        self.net = KeypointNet(values=values, depth_multiplier=self.params['depth_multiplier'], dtype=dtype, device=device)
        self.net.cache_inference_affine = True      # inference only: the batch-norm affines change with the variables alone
        self.use_graph = True                       # the device side of a call replays from a hipGraph per image shape
        self._graphs = {}
        self._eager_batches, self._batch_assigners = {}, {}         # predict_batch: buffers of the eager path, PRN per slot count
        self._image_capacity = {}                                   # predict_images: buffer capacities per (b, h, w, threshold)
        # groundtruth=: how mpn_oks_match scores and cuts an image's detections (by-value launch arguments: part of the key)
        self.oks_score, self.oks_max_dets = 'box', pose_metrics.MAX_DETS
        self.retinanet = None
        if detector_path is not None:
            from ..retinanet import PersonDetectorNet
            head = _load(detector_path)
            self.retinanet = PersonDetectorNet(backbone=self.net)
            self.retinanet.cache_inference_affine = True    # as for the backbone; _run compares the variable versions
            own = set(self.retinanet.vars) | set(self.retinanet.stats)
            self.retinanet.load_state_dict({k: v for k, v in head.items() if k in own}, strict=True)
        self.assigner = None
        if prn_path is not None:
            from ..prn import PoseResidualNet
            from ..prn_inference import KeypointAssigner
            prn_net = PoseResidualNet(values=_load(prn_path), batch=self.params['max_boxes'], dtype=dtype, device=device)
            self.assigner = KeypointAssigner(prn_net)

    def _detect(self, feats, n, h, w):
        """RetinaNet head + NMS on the shared backbone features (create_pb.py:70-81)."""
        det = self.retinanet
        b = det._buffers(n, h, w)
        det.head_forward({k: feats[k] for k in ("c3", "c4", "c5")}, b, False)
        p = self.params
        return det.nms(b, p['score_threshold'], p['iou_threshold'], p['max_boxes'])

    def __call__(self, image, score_threshold=0.05, boxes=None, scores=None):
        """
        Arguments:
            image: a numpy uint8 array with shape [height, width, 3], that represents a RGB image.
            score_threshold: a float number.
            boxes, scores: person boxes [n,4] normalised (ymin, xmin, ymax, xmax) (+ scores [n]) from the caller INSTEAD of the
                RetinaNet head's (for models without a detector_path); not part of the reference's signature.
        Returns the reference's dict (inference/detector.py:49-61): 'boxes' [n,4], 'scores' [n], 'num_boxes' (the graph's
        count before the score filter), 'keypoint_heatmaps' [h/4,w/4,17], 'segmentation_masks' [h/4,w/4],
        'keypoint_scores' [n,17], 'keypoint_positions' [n,17,2].
        """
        h, w, _ = image.shape
        assert h % 128 == 0 and w % 128 == 0                      # inference/detector.py:45
        if image.dtype != np.uint8:
            raise ValueError("image must be uint8")
        net = self.net
        if boxes is None and self.use_graph:
            dev = self._replay(image)
        else:
            dev = self._device_side(torch.from_numpy(np.ascontiguousarray(image[None])).to(net.device), boxes is None)
        heat, seg = dev['heat'], dev['seg']
        out = {'keypoint_heatmaps': heat[0].cpu().numpy(), 'segmentation_masks': seg[0].cpu().numpy()}
        kscore, kpos = np.zeros([0, 17], np.float32), np.zeros([0, 17, 2], np.float32)
        if boxes is not None:
            gb = np.asarray(boxes, np.float32).reshape(-1, 4)
            gs = np.ones(len(gb), np.float32) if scores is None else np.asarray(scores, np.float32)
            n = len(gb)
            if n and self.assigner is not None:
                dboxes = torch.from_numpy(gb[None]).to(net.device)
                ks, kp = self.assigner(heat.contiguous(), dboxes, torch.tensor([n], device=net.device), compact=True)
                kscore, kpos = ks.cpu().numpy(), kp.cpu().numpy()
        elif 'pred' in dev:
            pred = self.retinanet.check_nms(dev['pred'])
            n = int(pred['num_boxes'][0].item())
            gb, gs = pred['boxes'][0, :n].cpu().numpy(), pred['scores'][0, :n].cpu().numpy()
            if n and 'kscore' in dev:       # the padded slots (>= n) hold the results of zero crops: drop them
                kscore, kpos = dev['kscore'][:n].cpu().numpy(), dev['kpos'][:n].cpu().numpy()
        else:
            n = 0
            gb, gs = np.zeros([0, 4], np.float32), np.zeros([0], np.float32)
        keep = gs > score_threshold                                # inference/detector.py:54-59
        out.update({'boxes': gb[keep], 'scores': gs[keep], 'num_boxes': np.int32(n),
                    'keypoint_scores': kscore[keep] if len(kscore) else kscore,
                    'keypoint_positions': kpos[keep] if len(kpos) else kpos})
        return out

    def _device_side(self, x, detect):
        """Everything of create_pb.py:44-153 that runs on the device, static shapes throughout (the PRN runs on all max_boxes
        slots: padding slots are zero crops, dropped on the host): {'heat', 'seg'[, 'pred'[, 'kscore', 'kpos']]}."""
        net = self.net
        _, h, w, _ = x.shape
        bufs = net._buffers(1, h, w)
        feats = net.backbone_forward(x, False, bufs)               # uint8 -> /255 -> 2x-1 fused into the stem conv; ONE pass
        heat, seg = net.subnet_forward(feats, False, bufs, inference_outputs=True)
        dev = {'heat': heat, 'seg': seg}
        if detect and self.retinanet is not None:
            pred = self._detect(feats, 1, h, w)
            dev['pred'] = pred
            if self.assigner is not None:
                dev['kscore'], dev['kpos'] = self.assigner(heat.contiguous(), pred['boxes'], pred['num_boxes'], compact=False)
        return dev

    def _replay(self, image):
        """The device side of a call from a hipGraph captured once per image shape (an eager call first: it sizes the buffers and
        sets kernel attributes); the host copies the image into the graph's input and reads its outputs."""
        h, w, _ = image.shape
        held = self._graphs.get((h, w))
        ent = held[1] if held else _Entry(x=torch.empty((1, h, w, 3), dtype=torch.uint8, device=self.net.device))
        ent.x.copy_(torch.from_numpy(np.ascontiguousarray(image[None])))
        outs = self._run(ent, lambda: self._device_side(ent.x, True))
        if held is None:
            self._graphs[(h, w)] = [ent.graph, ent]     # element 0 is the graph: bench_legs.joint_inference_benchmark reads it there
        return outs

    def _run(self, ent, device_side):
        """The one capture / replay state machine of every predict path. device_side() queues the device work of a call over
        the entry's buffers and returns its outputs. use_graph False: just that. Else the first call of an entry runs it
        eagerly (the warm-up sizes the buffers, sets kernel attributes and fills the inference caches), synchronises and
        captures it over this call's data; every call then replays the graph."""
        ver = self._variable_versions()
        if not self.use_graph:
            return device_side()
        if ent.graph is None:
            device_side()
            torch.cuda.synchronize(self.net.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ent.outs = device_side()
            ent.graph, ent.ver = graph, ver
        elif ent.ver != ver:
            # variables changed since this graph last ran (load_state_dict, a train step on the shared backbone ...): the
            # batch-norm affines and the cast operands the captured launches read are host-cached and NOT in the graph. One
            # eager pass refreshes them through the normal code path into the same persistent buffers the graph reads.
            device_side()
            ent.ver = ver
        ent.graph.replay()
        return ent.outs

    # ------------------------------------------------------------------ batched inference
    def predict_batch(self, images, score_threshold=0.05, return_heatmaps=True, annotate=False, jpeg_quality=75,
                      jpeg_subsampling='4:2:0', plot_maps=False, groundtruth=None, flip=False, scales=None, track=None, track_style=None,
                      pose_nms=None, anonymize=None, crops=None, density=None, trails=None, zones=None, track_eval=None):
        """The joint graph over a BATCH (create_pb.py:16,53-61,96-109 are written for one), results packed on the device.

        Arguments:
            images: a numpy uint8 array [b, height, width, 3], or a list of b equally sized [height, width, 3] arrays.
            score_threshold: a float number (part of the captured graph: one graph per (b, height, width, threshold)).
            return_heatmaps: False omits 'keypoint_heatmaps' and 'segmentation_masks'; they then never leave the device.
            annotate: True adds 'annotated', a uint8 [height, width, 4] RGBA array: the image with that dict's persons drawn on
                it as inference/predict.ipynb's `draw_everything` draws them under Pillow, byte for byte (drawn on the device
                inside the captured graph: a graph of its own per (b, height, width, threshold)). 'jpeg' adds
                'annotated_jpeg' instead: that frame (its RGB) as the `bytes` of the JPEG file Pillow writes for it with
                `save(buf, "JPEG", quality=jpeg_quality, subsampling=jpeg_subsampling)`, encoded on the device inside the
                graph where the frame lies; only the compressed bytes are copied to the host.
            jpeg_quality, jpeg_subsampling: 1..100 and '4:4:4', '4:2:2' or '4:2:0'. The quality travels in descriptors: another
                quality replays the same graph; the sampling is part of the graph's key.
            plot_maps: True adds 'maps', a uint8 [18 * (height // 2), width // 2, 4] RGBA array: inference/predict.ipynb's
                `plot_maps` of the image, its heatmaps normalised per channel as the notebook normalises them, and its
                segmentation mask, byte for byte what Pillow and matplotlib make of them (made on the device inside the
                captured graph, a graph of its own; only the picture is copied to the host, with return_heatmaps False too).
                Combines freely with annotate.
            groundtruth: a list of b ground-truth dicts (pose_metrics.groundtruth_arrays: 'keypoints' [g,17,3] (x, y, v) and
                'boxes' [g,4] (x, y, w, h) in the pixels of the network input, optional 'area' and 'iscrowd'; at most 64
                persons each). Adds 'oks' to every dict: COCO's keypoint matching of that image's persons against its ground
                truth (`pose_metrics.PoseEvaluator.update` takes the dicts as they are), made by one mpn_oks_match launch
                behind the gather inside the captured graph - a graph of its own per (b, height, width, threshold,
                self.oks_score, self.oks_max_dets) that follows each call's ground truth; every other key is unchanged.
            flip: True averages every image's heatmaps and mask with those of its mirror image (test-time augmentation): the
                backbone and the keypoint subnet run once over 2b images, the second half mirrored on the device; the mirror's
                maps are un-mirrored (columns reversed, left / right keypoint channels swapped) and ONE mpn_tta_merge launch
                averages them into the maps that the PRN, plot_maps, 'keypoint_heatmaps' and 'segmentation_masks' then read.
                Boxes come from the unmirrored pass alone. A graph of its own; the averaged maps never leave the device
                unless return_heatmaps asks for them.
            scales: a list of at most 3 further network input sizes (width, height), multiples of 128 with the images' aspect
                ratio: the batch is resized to each on the device (mpn_image_resize: Pillow's bicubic), backbone and subnet
                run at that size (over the mirrors too with flip), and the maps are resized to the base size (bilinear,
                half-pixel centres) and averaged in the same launch, in the order base, base mirrored, scale 1, scale 1
                mirrored, ... (include/mpn.h states the arithmetic). Part of the graph's key, like flip.
            track: a tracking.PoseTracker. The images are frames of its streams (stream s owns images s*F .. s*F+F-1 in time
                order, b = streams * F). Adds 'track_ids' int32 [n] (a person's identity across the frames and calls of its
                stream, 0 = untracked), 'track_hits' int32 [n], 'track_new' bool [n] and 'track_similarity' f64 [n] to
                every dict: one mpn_pose_track launch behind the gather inside the captured graph - a graph of its own per
                (tracker, b) - whose rows arrive with the record. The launch only reads the tracker's state; the call
                advances it once, by a small device copy behind the graph. Every other key is unchanged. A tracker made
                with smooth=OneEuro(...) (needs the PRN) also adds 'keypoints_smoothed' f32 [n, 17, 3] - the One-Euro filtered
                (x, y) of every tracked person's joints with the frame's score, in the coordinates of this call's 'keypoints' -
                and 'keypoint_velocities' f32 [n, 17, 2] in pixels per second: one mpn_pose_smooth launch behind the track
                launch in the same graph, its rows in the same copy. A tracker made with motion=ConstantVelocity(...) matches
                against the tracks' predicted poses (mpn_pose_track_motion in place of mpn_pose_track) and adds 'coasting_ids' int32
                [m], 'coasting_misses' int32 [m], 'coasting_boxes' f32 [m, 4] and 'coasting_keypoints' f32 [m, 17, 2]: the tracks of
                the image's stream that are alive but were not detected in it, at their predicted pose, in the coordinates of this
                call's 'boxes' and 'keypoints'; the rows lie behind the others in the same copy. Without `track_style`, `annotate` still draws the frame's own
                detections in red and white.
            track_style: None, or an inference.TrackStyle (needs annotate and track): 'annotated' / 'annotated_jpeg' then carry
                the identities - mpn_draw_tracks in place of mpn_draw_detections, on the record, the track rows and (for
                keypoints='smoothed') the smoothed rows the graph has just produced: every tracked person's box, dots and an
                id label in the colour of its track, untracked persons as before or hidden. The style is part of the
                graph's key; its table goes to the device once, when the entry is made. None changes nothing.
            pose_nms: None, or an inference.PoseNms (needs the detector and the PRN, max_boxes <= 64): keypoint-similarity NMS
                of every image's persons. The gather writes its record to a device buffer of the entry that never leaves
                the device; one mpn_pose_nms behind it inside the captured graph - a graph of its own per PoseNms - writes
                the filtered record where the record lies otherwise, so that groundtruth=, track=, annotate= and the JPEG
                encoder read the surviving persons with no change of their own. Every dict then holds only the survivors
                and gains 'pose_nms_source' int32 [n] (a survivor's index among the image's persons before the stage),
                'pose_nms_absorbed' int32 [n] (the persons it suppressed) and 'pose_nms_suppressed' (np.int32); they arrive
                in the record's one copy. 'num_boxes' is still the count before the score filter. None changes nothing.
            track_eval: None, or a track_metrics.TrackEvaluator (needs track=, the PRN and a groundtruth= whose dicts carry
                'track_ids'; the evaluator's streams and max_boxes are the tracker's, its max_gt 64): one mpn_track_eval launch
                behind the tracker's inside the captured graph - a graph of its own per evaluator - scores the identities
                against the annotated ones over the record the tracker read (the filtered one with pose_nms=). The ground-truth
                rows are those groundtruth= placed; the identity indices go up in one more small copy; the rows lie behind
                every other part of the result buffer and arrive in the record's one copy. The launch only reads the
                evaluator's state; the call advances it once, beside the tracker's. Every dict gains 'track_eval'
                (`TrackEvaluator.unpack`: the frame's counts, per ground truth the matched id, flags and similarity, per
                person the matched ground truth and flags); `evaluator.collect(outputs)` feeds `evaluate()`. None changes nothing.
            trails: None, or a trails.TrackTrails (needs track=; its streams and max_boxes are the tracker's, its frame_size the
                size of the frames): one mpn_track_trails launch behind the tracker's (and mpn_zone_events) inside the captured
                graph - a graph of its own per TrackTrails - keeps every identity's last anchors over the record the tracker
                read. The rows lie at the very end of the result buffer and arrive in the record's one copy; the launch only
                reads the state, the call advances it once, beside the tracker's. Every dict gains 'trails'
                (`TrackTrails.unpack`: per person its points, newest first, their count and flags). With annotate and
                `trails.draw`, mpn_draw_trails blends the polylines into the annotated frame before it is encoded (not with
                anonymize's overlay=False, which draws nothing). Coasting tracks add no points. None changes nothing.
            density: None, or a density.DensityMap (track= is optional; with it the map's streams are the tracker's; its
                max_boxes is the Detector's, its frame_size the size of the frames): one mpn_density_map launch behind the tracker's
                (and mpn_track_trails) inside the captured graph - a graph of its own per DensityMap - adds every kept person to
                the cell it stands in: the dwell plane, and with track= the visits plane. The rows lie at the very end of the
                result buffer and arrive in the record's one copy; the launch only reads the state, the call advances it once,
                beside the tracker's. Every dict gains 'density' (`DensityMap.unpack`: per person its cell and flags, per frame the
                maxima and counts); `density.grid()` reads a plane. With annotate and `density.draw`, mpn_draw_density blends
                the map over the annotated frame before it is encoded (not with anonymize's overlay=False, which draws nothing).
                Persons below score_threshold and coasting tracks are not counted. None changes nothing.
            zones: None, or a zones.ZoneCounter (needs track=; the counter's streams and max_boxes are the tracker's, its
                frame_size the size of the frames): one mpn_zone_events launch behind the tracker's inside the captured graph - a
                graph of its own per counter - tests every kept person's anchor (the feet; without the PRN the box) against the
                counter's polygons and lines over the record the tracker read (the filtered one with pose_nms=). The rows lie
                behind every other part of the result buffer and arrive in the record's one copy. The launch only reads the
                counter's state; the call advances it once, beside the tracker's. Every dict gains 'zones'
                (`ZoneCounter.unpack`: per person the zones it is inside, its entries, exits, line crossings, anchor and dwell
                times; per frame the occupancy, the events and the running totals). Persons below score_threshold and coasting
                tracks are not counted. Every other key is unchanged. None changes nothing.
            anonymize: None, or an inference.Anonymize (needs annotate=True or 'jpeg' and the detector; max_boxes <= 128): every
                kept person is made unrecognisable in the frame `annotate` shows - its head, from the record's face joints, or
                its box, pixelated, blurred or filled. One mpn_anonymize behind the gather (behind mpn_pose_nms: on the
                survivors) inside the captured graph - a graph of its own per Anonymize - writes the anonymised frames to a
                buffer of the entry; the drawing takes that buffer as its sources, so boxes, skeletons and identities lie over
                the mosaic ('annotated', 'annotated_jpeg'). With overlay=False nothing is drawn: the anonymised frame alone,
                alpha 255 (not with track_style). Without the PRN every person takes the fallback region. Every other key is
                unchanged; `plot_maps` and the returned heatmaps still show the network's input, NOT the anonymised frame.
                None changes nothing.
            crops: None, or an inference.PersonCrops (needs the detector; its max_boxes is the Detector's, at most 128): the
                picture of every kept person, cut from its frame and resized to the spec's size as Pillow's bicubic
                `resize(box=...)` does it, byte for byte. One mpn_person_crops behind the gather (behind mpn_pose_nms: the
                survivors) and behind mpn_anonymize inside the captured graph - a graph of its own per PersonCrops - builds the
                tap tables of every crop on the device from the record's boxes and writes the crops to a buffer of the
                entry; with format='jpeg' the encoder's two launches follow it there. It reads the frames the drawing reads
                as its sources - the batch; with anonymize= the ANONYMISED buffer, never the overlays, so that no
                un-anonymised pixel leaves through this key - and does not need annotate. Every dict gains 'crops' - uint8
                [n, H, W, 3], or with format='jpeg' a list of n `bytes` - entry i the person i of 'boxes' (the filtered
                order with pose_nms=), and 'crop_info': 'rect' f64 [n, 4] (x0, y0, x1, y1) in the frame's pixels, 'placed'
                int32 [n, 4] (top, left, new_h, new_w) inside the crop and 'empty', 'too_large' (a reduction beyond 16x),
                'clipped' bool [n]; an empty or too large crop is all `fill`. The fixed-size info block arrives with the
                record; exactly the used crops, or their streams, follow in one more copy. Every other key is unchanged.
                None changes nothing.
        Returns a list of b dicts, dict i holding what `__call__` returns for image i (the same keys, shapes and dtypes) plus
        'keypoints' [n, 17, 3]: (x, y, score) in image pixels (inference/predict.ipynb, draw_everything, in float32).
        """
        opts, (b, h, w) = self._options(
            lambda: check_batch(images), score_threshold=score_threshold, return_heatmaps=return_heatmaps, annotate=annotate,
            jpeg_quality=jpeg_quality, jpeg_subsampling=jpeg_subsampling, plot_maps=plot_maps, groundtruth=groundtruth, flip=flip,
            scales=scales, track=track, track_style=track_style, pose_nms=pose_nms, track_eval=track_eval, anonymize=anonymize, zones=zones, trails=trails, density=density, crops=crops)
        # pinned staging; the frames are the batch itself, so the drawing and encode descriptors are fixed with the entry
        ent = self._entry(opts, (b, h, w, opts.thr) if self.use_graph else ('eager', b, h, w), (b, h, w),
                          lambda: _Entry(stage=torch.empty((b, h, w, 3), dtype=torch.uint8).pin_memory()),
                          (b * h * w * 3,), fixed_frames=True)
        if opts.oks:
            ent.oks.place(groundtruth)                              # ONE small host-to-device copy of the ground truth
        if ent.track_eval is not None:                              # one more small copy: the identity indices
            ent.track_eval.place(groundtruth, b, rows=False)
        if opts.jpeg and ent.encode_plan.quality != opts.jpeg[0]:   # the frames are fixed: only another quality needs new descriptors
            self._place_encode(ent, _encode_plan(*_batch_frames(b, h, w), opts.jpeg))
        stage = ent.stage.numpy()
        if isinstance(images, np.ndarray):
            stage[...] = images
        else:
            for i, im in enumerate(images):
                stage[i] = im
        ent.x[:b].copy_(ent.stage, non_blocking=True)               # ONE host-to-device copy
        outs = self._run(ent, lambda: self._device_side_batch(ent, opts.thr))
        ent.commit()
        return self._finish(ent, outs, b, opts.return_heatmaps)

    def _options(self, shape, **given):
        """Every argument check of the predict_* methods, in one order and before any device work -> (_Options, what shape()
        returned). given: the keywords the three methods share, as they came (pose_nms, track_eval, density, trails, zones and
        anonymize may be absent: None). shape(): the method's own checks of its images and sizes, run behind those of
        annotate, track_style and plot_maps; what it returns begins with (b, height, width) of the network input. The order
        behind it: groundtruth, track, flip / scales, pose_nms, track_eval, density, trails, zones, anonymize, crops."""
        jp = check_annotate(given['annotate'], given['jpeg_quality'], given['jpeg_subsampling'])
        style = check_track_style(given['track_style'], given['annotate'], given['track'])
        plot_maps = check_plot_maps(given['plot_maps'], self._has_heatmaps)
        shaped = shape()
        b, h, w = shaped[:3]
        thr = float(given['score_threshold'])
        oks = self._check_groundtruth(given['groundtruth'], b)
        self._check_track(given['track'], b)
        tta_key = check_tta(given['flip'], given['scales'], h, w)
        if tta_key and not self._has_heatmaps():
            raise ValueError("flip / scales average the keypoint subnet's heatmap outputs; this Detector has none")
        nms = self._check_pose_nms(given.get('pose_nms'))
        evaluator = self._check_track_eval(given.get('track_eval'), given['track'], given['groundtruth'], b)
        sizes = shaped[4].sizes if len(shaped) > 4 else [(h, w)]
        density = self._check_density(given.get('density'), given['track'], b, sizes)
        trails = self._check_rider('trails', given.get('trails'), given['track'], b, sizes)
        counter = self._check_rider('zones', given.get('zones'), given['track'], b, sizes)
        spec = self._check_anonymize(given.get('anonymize'), given['annotate'], given['track_style'])
        cut = self._check_crops(given.get('crops'), b)
        return _Options(thr, jp or bool(given['annotate']), plot_maps, oks, tta_key, given['track'], style,
                        given['return_heatmaps'], evaluator, cut, density, trails, counter, spec, nms), shaped

    def _check_fit(self, keyword, noun, stage, track=None, limits=None):
        """What every stateful stage must share with this Detector, in one order: the streams of the tracker it rides on (where
        there is one), max_boxes, `limits()` - a stage's own sizes - and the device. noun: what the messages call the stage (one that ends in s is a
        plural: "the trails were made for ...")."""
        was, lives = ('were', 'live') if noun.endswith('s') else ('was', 'lives')
        if track is not None and stage.streams != track.streams:
            raise ValueError(f"{keyword}=: {noun} {was} made for {stage.streams} streams, the tracker for {track.streams}")
        if stage.max_boxes != self.params['max_boxes']:
            raise ValueError(f"{keyword}=: {noun} {was} made for max_boxes = {stage.max_boxes}, this Detector's is "
                             f"{self.params['max_boxes']}")
        if limits is not None:
            limits()
        if torch.device(stage.device) != torch.device(self.net.device):
            raise ValueError(f"{keyword}=: {noun} {lives} on {stage.device}, this Detector on {self.net.device}")

    def _check_rider(self, keyword, stage, track, b, sizes=None, rules=None, limits=None):
        """The `track_eval`, `zones`, `trails` or `density` argument of the predict_* methods, a stage that rides on the tracker
        -> None or the stage. In one order: its type; that there is a tracker (where `_RIDERS` says why it needs one) and
        `rules()`, the stage's own about the detector, the PRN and the other keywords; `_check_fit`; sizes, the (height, width)
        of the call's frames, in whose pixels the record's keypoints are, against the stage's frame_size; `out_bytes(b)`. Before
        any device work."""
        if stage is None:
            return None
        module, cls, noun, why = _RIDERS[keyword]
        if not isinstance(stage, getattr(importlib.import_module('..' + module, __package__), cls)):
            raise ValueError(f"{keyword} must be None or a {module}.{cls}")
        if why is not None and track is None:
            raise ValueError(f"{keyword}= {why}: it needs track=, a tracking.PoseTracker")
        if rules is not None:
            rules()
        self._check_fit(keyword, noun, stage, track, limits)
        if sizes is not None:
            stage.check_frame_sizes(sizes)
        stage.out_bytes(b)
        return stage

    def _check_density(self, density, track, b, sizes):
        """The `density` argument: `_check_rider` with its own rules - track= is optional, show='visits' needs it."""
        def rules():
            if self.retinanet is None:
                raise ValueError("density= counts the persons of the record: this Detector has no person detector")
            if track is None and density.show == 'visits':
                raise ValueError("density=: show='visits' counts the arrivals of identities: it needs track=, a tracking.PoseTracker")
        return self._check_rider('density', density, track, b, sizes, rules)

    def _check_anonymize(self, spec, annotate, track_style):
        """The `anonymize` argument of the predict_* methods -> None or the Anonymize. Before any device work."""
        if spec is None:
            return None
        anonymize_stage.check_spec(spec)
        if not annotate:
            raise ValueError("anonymize= changes the frame annotate shows: it needs annotate=True or 'jpeg'")
        if not spec.overlay and track_style is not None:
            raise ValueError("anonymize: overlay=False draws nothing over the anonymised frame; track_style= says how to draw")
        if self.retinanet is None:
            raise ValueError("anonymize= needs the person detector (detector_path): without it no persons are detected")
        anonymize_stage.check_max_boxes(self.params['max_boxes'])
        return spec

    def _check_crops(self, spec, b):
        """The `crops` argument of the predict_* methods -> None or the PersonCrops. Before any device work."""
        if spec is None:
            return None
        crops_stage.check_spec(spec)
        if self.retinanet is None:
            raise ValueError("crops= needs the person detector (detector_path): without it no persons are detected")
        if spec.max_boxes != self.params['max_boxes']:
            raise ValueError(f"crops=: the PersonCrops was made for max_boxes = {spec.max_boxes}, this Detector's is "
                             f"{self.params['max_boxes']}")
        if b * spec.max_boxes > 4096:
            raise ValueError(f"crops=: {b} x {spec.max_boxes} slots are more than mpn_person_crops takes in one launch (4096)")
        return spec

    def _check_track_eval(self, evaluator, track, groundtruth, b):
        """The `track_eval` argument: `_check_rider` with its own rules (before the evaluator gives an identity a dense index)."""
        def rules():
            from ..track_metrics import groundtruth_track_ids
            if groundtruth is None:
                raise ValueError("track_eval= needs groundtruth=, a list of dicts that carry 'track_ids'")
            if self.assigner is None:
                raise ValueError("track_eval= compares keypoints, which need the PRN (prn_path)")
            for gt in groundtruth:
                groundtruth_track_ids(gt, len(pose_metrics.groundtruth_arrays(gt)[0]))

        def limits():
            if evaluator.max_gt != pose_metrics.MAX_GT:
                raise ValueError(f"track_eval=: the Detector's ground-truth rows are {pose_metrics.MAX_GT} per image; make the "
                                 f"evaluator with max_gt = {pose_metrics.MAX_GT} (got {evaluator.max_gt})")
        return self._check_rider('track_eval', evaluator, track, b, rules=rules, limits=limits)

    def _check_pose_nms(self, nms):
        """The `pose_nms` argument of the predict_* methods -> None or the PoseNms. Before any device work."""
        if nms is None:
            return None
        if not isinstance(nms, pose_nms_stage.PoseNms):
            raise ValueError("pose_nms must be None or an inference.PoseNms")
        if self.retinanet is None:
            raise ValueError("pose_nms= needs the person detector (detector_path): without it no persons are detected")
        if self.assigner is None:
            raise ValueError("pose_nms= compares keypoints, which need the PRN (prn_path)")
        pose_nms_stage.check_max_boxes(self.params['max_boxes'])
        return nms

    def _check_groundtruth(self, groundtruth, b):
        """The `groundtruth` argument of the predict_* methods -> () or the tail of the entry's key."""
        if groundtruth is None:
            return ()
        if self.retinanet is None:
            raise ValueError("groundtruth= needs the person detector (detector_path): without it no persons are detected")
        if not isinstance(groundtruth, (list, tuple)) or len(groundtruth) != b:
            raise ValueError(f"groundtruth must be a list of {b} dicts, one per image")
        if self.oks_score not in pose_metrics.SCORE_MODES:
            raise ValueError(f"oks_score must be one of {sorted(pose_metrics.SCORE_MODES)} (got {self.oks_score!r})")
        return ('oks', self.oks_score, int(self.oks_max_dets))

    def _check_track(self, track, b):
        """The `track` argument of the predict_* methods: raises unless it is None or a tracker this Detector can run over b
        images. Before any device work."""
        if track is None:
            return
        from ..tracking import PoseTracker
        if not isinstance(track, PoseTracker):
            raise ValueError("track must be a tracking.PoseTracker")
        if self.retinanet is None:
            raise ValueError("track= needs the person detector (detector_path): without it no persons are detected")
        if track.similarity == 'oks' and self.assigner is None:
            raise ValueError("track=: similarity='oks' compares keypoints, which need the PRN (prn_path); use similarity='iou'")
        if track.smooth is not None and self.assigner is None:
            raise ValueError("track=: the tracker's smooth= filters keypoints, which need the PRN (prn_path)")
        track.check_batch(b)
        self._check_fit('track', 'the tracker', track)
        track.out_bytes(b)

    @staticmethod
    def _place_encode(ent, plan):
        """This call's encode descriptors (geometry, offsets, quantisation tables) go to the device: one small copy."""
        ent.encode_plan = plan
        ent.encode.upload(plan)

    def _finish(self, ent, outs, b, return_heatmaps):
        """The host side behind the device side of predict_batch / predict_images: the record (and the maps) into pinned
        memory, one synchronise, the record unpacked into b dicts. With crops= the info block comes with the record; the used
        crops follow in a second step (`crops.CropBuffers.collect`), the shape `JpegBatchEncoder.collect` has."""
        copies = [('record', outs.get('record'))]
        if return_heatmaps:
            copies += [('heat', outs['heat']), ('seg', outs['seg'])]
        if 'maps' in outs:
            copies.append(('maps', outs['maps']))
        for name, src in copies:                                    # ONE device-to-host copy each, into pinned memory
            if src is None:
                continue
            if name not in ent.host:
                ent.host[name] = torch.empty(src.shape, dtype=src.dtype).pin_memory()
            ent.host[name].copy_(src, non_blocking=True)
        if 'annotated' in outs:                                     # this batch's bytes of the packed frames, not the capacity
            if 'annotated' not in ent.host:
                ent.host['annotated'] = torch.empty(outs['annotated'].shape, dtype=torch.uint8).pin_memory()
            nb = ent.draw.out_bytes
            ent.host['annotated'][:nb].copy_(outs['annotated'][:nb], non_blocking=True)
        if 'crops' in outs:                                         # the fixed-size info block, with the record
            ent.crops.fetch_info()
        torch.cuda.current_stream(self.net.device).synchronize()
        host = ent.host
        files = ent.encode.collect(ent.encode_plan, outs['encoded']) if 'encoded' in outs else None
        if 'record' in outs:
            record = host['record'].numpy()
            persons = unpack_record(record, b, self.params['max_boxes'], self.assigner is not None)
            counts = record[4:4 + 4 * b].view(np.int32)
            for st in _STAGES:                                      # every stage's rows lie behind the record: they came with it
                stage = getattr(ent, st.part)
                if stage is None:
                    continue
                for p, rows in zip(persons, stage.unpack(record[getattr(ent.layout, st.part)], counts)):
                    if st.result is None:
                        p.update(rows)
                    else:
                        p[st.result] = rows
            if 'crops' in outs:                                     # exactly the used crops (or their streams): one more step
                for p, (cut, info) in zip(persons, ent.crops.collect([len(p['boxes']) for p in persons])):
                    p['crops'], p['crop_info'] = cut, info
        else:                                                       # no detector_path: no boxes are detected
            persons = [_no_persons() for _ in range(b)]
        if return_heatmaps:
            heat, seg = host['heat'].numpy().copy(), host['seg'].numpy().copy()
            for i, p in enumerate(persons):
                p['keypoint_heatmaps'], p['segmentation_masks'] = heat[i], seg[i]
        if 'annotated' in outs:
            for p, frame in zip(persons, ent.draw.unpack(host['annotated'].numpy())):
                p['annotated'] = frame
        if files is not None:
            for p, data in zip(persons, files):
                p['annotated_jpeg'] = data
        if 'maps' in outs:
            for p, frame in zip(persons, host['maps'].numpy().copy()):
                p['maps'] = frame
        return persons

    def _entry(self, opts, base, shape, make, capacity, fixed_frames=False):
        """The entry of one key, base + opts.tail(b), in `_graphs` (use_graph False: `_eager_batches`), made on its first use
        (`_run` adds the captured graph). make(): an _Entry with the staging and device buffers of the path. To it come the
        device input for shape = (b, h, w) (with the mirrors behind the batch and the inputs of the extra scales for flip /
        scales), what each option needs (`_Entry`) - the drawing's buffers sized for sources of capacity[0] bytes, the JPEG
        encoder reserving capacity[1:], the style's table, which goes to the device once, here - and the layout of the result
        buffer. fixed_frames (predict_batch): the frames are the batch itself, so the drawing and encode descriptors are
        placed here, for good, and the encoder reserves what their plan needs."""
        b, h, w = shape
        key = base + opts.tail(b)
        store = self._graphs if self.use_graph else self._eager_batches
        ent = store.get(key)
        if ent is not None:
            return ent
        dev = self.net.device
        ent = make()
        if opts.tta:
            ent.tta = tta.Buffers(opts.tta[1], opts.tta[2], b, h, w, dev)
            ent.x = ent.tta.x
        else:
            ent.x = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev)
        if opts.annotate:
            ent.draw = draw.Buffers(b, self.params['max_boxes'], capacity[0], dev)
            if fixed_frames:
                ent.draw.place(*_batch_frames(b, h, w))
        if opts.anonymize is not None:                              # its output is a buffer like the sources
            ent.anonymize = anonymize_stage.Anonymizer(b, self.params['max_boxes'], capacity[0], dev, opts.anonymize)
            if fixed_frames:
                ent.anonymize.place(*_batch_frames(b, h, w))
        if opts.crops is not None:                                  # the crops, their info block, taps and (jpeg) encoder
            ent.crops = crops_stage.CropBuffers(b, self.params['max_boxes'], opts.crops, dev)
            if fixed_frames:
                ent.crops.place(*_batch_frames(b, h, w))
        if opts.jpeg:                                               # the frames lie where the drawing writes them
            plan = _encode_plan(*_batch_frames(b, h, w), opts.jpeg) if fixed_frames else None
            ent.encode = jpeg.JpegBatchEncoder(dev)
            ent.encode.reserve(b, *(plan.need if plan else capacity[1:]))
            if plan:
                self._place_encode(ent, plan)
        if opts.plot_maps:
            ent.maps = maps.MapPlotter(b, h, w, h // 4, w // 4, dev)
        if opts.oks:
            ent.oks = pose_metrics.OksBuffers(b, self.params['max_boxes'], pose_metrics.MAX_GT, dev, opts.oks[1], opts.oks[2])
        if opts.pose_nms is not None:
            ent.nms = pose_nms_stage.PoseNmsBuffers(b, self.params['max_boxes'], opts.pose_nms, dev)
        for st in _STAGES:
            if st.stateful:
                setattr(ent, st.part, getattr(opts, st.option))
        ent.layout = RecordLayout(b, self.params['max_boxes'], **{st.part: getattr(ent, st.part) for st in _STAGES})
        if opts.style:
            ent.style = opts.style[1], torch.from_numpy(opts.style[1].tables().copy()).to(dev)
        store[key] = ent
        return ent

    def _device_side_batch(self, ent, score_threshold, extent=None, frames=None):
        """_device_side for the b images of the entry's input ent.x, then mpn_pose_gather: {'heat', 'seg'[, 'record']}. The PRN
        runs ONCE over all b * max_boxes slots (an instance of that batch size on the shared variables). extent
        (predict_images): f32 [b, 4] on the device; the gather is then mpn_pose_gather_sized, which maps boxes and keypoints to
        the source images. frames: the flat uint8 sources the drawing reads (default: the batch x itself).
        What the entry holds decides the rest (`predict_batch` describes every option, DESIGN.md "The row stages of the
        Detector" the order): ent.tta - mirrors, extra scales and ONE mpn_tta_merge, whose maps everything below reads;
        ent.maps -> 'maps'; behind the gather the launches that write rows into the one result buffer where `ent.layout` says
        (-> 'record', the whole buffer): pose_nms, whose filtered record every later launch reads, oks, track, track_eval,
        zones, trails, density; then anonymize, the crops (mpn_person_crops over the frames the drawing reads -> 'crops', with
        format='jpeg' encoded behind it), the drawing (mpn_draw_tracks with ent.style), mpn_draw_trails and
        mpn_draw_density over its frames in place (-> 'annotated') and the JPEG encode (-> 'encoded' instead). Every launch is
        a pure function of its inputs and the stages' previous state: `_run` may launch twice, the caller commits once."""
        net = self.net
        x, annotate, aug, track = ent.x, ent.draw, ent.tta, ent.track
        if aug is not None and aug.flip:
            tta.mirror_images(x[:aug.b], x[aug.b:])
        heat, seg, feats = self._keypoint_pass(x)
        if aug is not None:
            b = aug.b
            sources = self._tta_sources(heat, seg, aug)
            for xk, meta, work in aug.scales:
                aug.fill(x, xk, meta, work)
                sources += self._tta_sources(*self._keypoint_pass(xk)[:2], aug)
            heat, seg = aug.heat, aug.seg
            tta.merge(sources, heat, seg)
            x = x[:b]                                               # N is the outermost axis: contiguous prefixes
            feats = {k: (raw[:b], aff) for k, (raw, aff) in feats.items()}
        b, h, w, _ = x.shape
        dev = {'heat': heat, 'seg': seg}
        if ent.maps is not None:
            dev['maps'] = ent.maps.launch(x, heat, seg, normalise=True)
        if (annotate is not None or ent.crops is not None) and frames is None:
            frames = x.view(-1)
        if self.retinanet is None:
            if annotate is not None:                                # no detector: the frames with alpha 255
                dev['annotated'] = annotate.launch(frames, None, False)
            return self._encode_frames(dev, ent.encode)
        pred = self._detect(feats, b, h, w)
        max_boxes = pred['boxes'].shape[1]
        kscore = kpos = None
        if self.assigner is not None:
            a = self._assigner_for(b * max_boxes)
            crops = a.crops_of_slots(heat, pred['boxes'], pred['num_boxes'], 0, b * max_boxes)
            kscore, kpos = a.decode(a.net.predict(crops))
        layout = ent.layout
        nbytes = layout.record.stop
        if nbytes == 0:
            raise ValueError(f"predict_batch: {b} x {max_boxes} slots are more than mpn_pose_gather packs in one launch")
        whole = torch.empty(layout.nbytes, dtype=torch.uint8, device=net.device)
        filtered = whole[layout.record]
        # the tracker's identity rows, which every stage behind it reads (its smoothed and coasting rows lie behind them)
        ids = whole[layout.track][:track.track_bytes(b)] if track is not None else None
        record = ent.nms.raw if ent.nms is not None else filtered    # what the gather writes
        if extent is None:
            _lib.call("mpn_pose_gather", _lib.ptr(pred['boxes']), _lib.ptr(pred['scores']), _lib.ptr(pred['num_boxes']), _lib.ptr(kscore),
                      _lib.ptr(kpos), _lib.ptr(pred['overflow']), b, max_boxes, float(score_threshold), h, w, _lib.ptr(record), nbytes,
                      _lib.stream_ptr())
        else:
            _lib.call("mpn_pose_gather_sized", _lib.ptr(pred['boxes']), _lib.ptr(pred['scores']), _lib.ptr(pred['num_boxes']),
                      _lib.ptr(kscore), _lib.ptr(kpos), _lib.ptr(pred['overflow']), b, max_boxes, float(score_threshold),
                      _lib.ptr(extent), _lib.ptr(record), nbytes, _lib.stream_ptr())
        if ent.nms is not None:                                     # every launch below reads the filtered record
            record = ent.nms.launch(filtered, whole[layout.nms])
        if ent.oks is not None:
            ent.oks.launch(record, whole[layout.oks])
        if track is not None:                                       # (with smooth=: mpn_pose_smooth behind it, rows behind its rows)
            track.launch_all(record, whole[layout.track], b)
        if ent.track_eval is not None:                              # the record the tracker read, its rows, the ground truth in place
            ent.track_eval.launch(record, ids, whole[layout.track_eval], b, *ent.oks.device_groundtruth())
        if ent.zones is not None:                                   # the record the tracker read and its rows; without the PRN: boxes
            ent.zones.launch(record, ids, whole[layout.zones], b, self.assigner is not None)
        if ent.trails is not None:                                  # likewise
            ent.trails.launch(record, ids, whole[layout.trails], b, self.assigner is not None)
        density_drawn = (ent.density is not None and annotate is not None and ent.density.draw and
                         (ent.anonymize is None or ent.anonymize.spec.overlay))
        if ent.density is not None:                                 # the same record; identities where there is a tracker
            ent.density.launch(record, ids, whole[layout.density], b, self.assigner is not None,
                               ent.density.snapshots(b) if density_drawn else None)
        dev['record'] = whole
        drawn = record
        if ent.anonymize is not None:                               # the drawing reads the anonymised frames in place of the sources
            frames = ent.anonymize.launch(frames, record, self.assigner is not None)
            if not ent.anonymize.spec.overlay:
                drawn = None                                        # (draw.Buffers.no_record: the frames with alpha 255)
        if ent.crops is not None:                                   # the sources of the drawing, never its overlays
            dev['crops'] = ent.crops.launch(frames, record)
        if annotate is not None and ent.style is not None:          # identities: mpn_draw_tracks on the rows just written
            style, table = ent.style
            smoothed = whole[layout.track][track.track_bytes(b):] if style.keypoints == 'smoothed' else None
            dev['annotated'] = annotate.launch_tracks(frames, record, ids, smoothed, table, self.assigner is not None)
        elif annotate is not None:
            dev['annotated'] = annotate.launch(frames, drawn, drawn is not None and self.assigner is not None)
        if annotate is not None and ent.trails is not None and ent.trails.draw and drawn is not None:
            # the polylines over the frames just written, in place, before they are encoded
            ent.trails.launch_draw(annotate.desc, record, ids, whole[layout.trails], dev['annotated'], b)
        if density_drawn:                                           # the map over everything drawn so far, in place
            ent.density.launch_draw(annotate.desc, ent.density.snapshots(b), whole[layout.density], dev['annotated'], b)
        return self._encode_frames(dev, ent.encode)

    def _keypoint_pass(self, x):
        """Backbone and keypoint subnet over a uint8 batch: (sigmoid heatmaps, mask, backbone features)."""
        net = self.net
        n, h, w, _ = x.shape
        bufs = net._buffers(n, h, w)
        feats = net.backbone_forward(x, False, bufs)
        heat, seg = net.subnet_forward(feats, False, bufs, inference_outputs=True)
        return heat, seg, feats

    @staticmethod
    def _tta_sources(heat, seg, aug):
        """The merge sources of one pass: its first b images plain, then (flip) its second b images as mirrored maps."""
        b = aug.b
        return [(heat[:b], seg[:b], False)] + ([(heat[b:], seg[b:], True)] if aug.flip else [])

    @staticmethod
    def _encode_frames(dev, encode):
        if encode is not None:
            dev['encoded'] = dev.pop('annotated')
            encode.launch(dev['encoded'])
        return dev

    # ------------------------------------------------------------------ ragged frames: on-device resize
    def predict_images(self, images, size=(640, 640), keep_aspect_ratio=False, score_threshold=0.05, return_heatmaps=False,
                       annotate=False, jpeg_quality=75, jpeg_subsampling='4:2:0', plot_maps=False, groundtruth=None,
                       flip=False, scales=None, track=None, track_style=None, pose_nms=None, anonymize=None, crops=None,
                       density=None, trails=None, zones=None, track_eval=None):
        """`predict_batch` for frames as a camera or a dataset delivers them: the resize of inference/predict.ipynb (cell 6:
        Pillow's `image.resize`, antialiased bicubic) runs on the device inside the captured graph, equal to Pillow byte for
        byte, and the persons come back in the coordinates of the SOURCE images (its `draw_everything`).

        Arguments:
            images: a list of b >= 1 uint8 arrays [h_i, w_i, 3]; the sizes may all differ and need not be multiples of anything.
            size: (height, width) of the network input, both multiples of 128.
            keep_aspect_ratio: False resizes every image to exactly `size` (the notebook). True resizes image i to
                new_h x new_w, s = min(height / h_i, width / w_i), new_h = max(1, round(h_i * s)), new_w = max(1, round(w_i * s))
                (float64, Python's `round`), placed at the top left of a zero canvas (`pad_to_bounding_box`).
            score_threshold: a float number (part of the captured graph).
            return_heatmaps: True adds 'keypoint_heatmaps' [height/4, width/4, 17] and 'segmentation_masks' of the network
                CANVAS and 'resized_size': (new_h, new_w), the part of the canvas the image covers.
            annotate: True adds 'annotated', a uint8 [h_i, w_i, 4] RGBA array: the SOURCE frame at its own size with that
                dict's persons drawn on it as inference/predict.ipynb's `draw_everything` draws them under Pillow, byte for
                byte (drawn on the device inside the captured graph, from the frames already uploaded for the resize).
                'jpeg' adds 'annotated_jpeg' instead, as `predict_batch` does: the file Pillow writes for that frame.
            jpeg_quality, jpeg_subsampling: as for `predict_batch`.
            plot_maps: as for `predict_batch`; the picture shows the network's input, the resized CANVAS (padding included).
            groundtruth: as for `predict_batch`, in the pixels of the SOURCE images (where 'keypoints' are returned).
            flip, scales: as for `predict_batch`, of the network CANVAS: its mirror (with keep_aspect_ratio the padding then
                lies on the other side) and the canvas resized to each (width, height) of `scales`, which have the aspect
                ratio of `size` - not the source frames resized again.
            track: as for `predict_batch`; the tracker sees the boxes normalised to the source images and the keypoints in
                source pixels, as they are returned.
            track_style: as for `predict_batch`; the identities are drawn on the SOURCE frames.
            pose_nms: as for `predict_batch`; the similarity is that of the keypoints in source pixels, as they are returned.
            track_eval: as for `predict_batch`, with the ground truth in the pixels of the SOURCE images.
            zones: as for `predict_batch`, in the pixels of the SOURCE images, which must all have the counter's frame_size.
            anonymize: as for `predict_batch`; the SOURCE frames are anonymised at their own size. `plot_maps` and the heatmaps
                still show the network's input.
            crops: as for `predict_batch`; the persons are cut from the SOURCE frames at their own size (the packed sources;
                with anonymize= the anonymised ones, never the overlays), 'rect' is in source pixels.
        Returns a list of b dicts with the keys of `predict_batch`: 'boxes' normalised to the source image, 'keypoints'
        (x, y, score) in source pixels; 'scores', 'num_boxes', 'keypoint_scores', 'keypoint_positions' as `predict_batch` gives
        them for the resized batch. A resize that needs more than resample.MAX_KSIZE taps per output (a reduction beyond 16x)
        raises ValueError.
        """
        def shape():
            items = resample.check_images(images)
            height, width = resample.check_size(size)
            return len(items), height, width, items, resample.Plan([im.shape[:2] for im in items], height, width, keep_aspect_ratio)
        opts, (_, _, _, items, plan) = self._options(
            shape, score_threshold=score_threshold, return_heatmaps=return_heatmaps, annotate=annotate, jpeg_quality=jpeg_quality,
            jpeg_subsampling=jpeg_subsampling, plot_maps=plot_maps, groundtruth=groundtruth, flip=flip, scales=scales,
            track=track, track_style=track_style, pose_nms=pose_nms, track_eval=track_eval, anonymize=anonymize, zones=zones, trails=trails, density=density, crops=crops)

        def upload(ent):
            stage = ent.stage.numpy()
            for im, at in zip(items, plan.src_offsets):
                stage[at:at + im.size] = im.reshape(-1)
            nb = plan.stage_bytes                                   # this batch's bytes, not the buffers' capacity
            ent.sources[:nb].copy_(ent.stage[:nb], non_blocking=True)       # ONE host-to-device copy of the frames
        return self._predict_sources(plan, upload, opts, groundtruth)

    # ------------------------------------------------------------------ ragged frames as JPEG bytes: on-device decode
    def predict_jpegs(self, jpegs, size=(640, 640), keep_aspect_ratio=False, score_threshold=0.05, return_heatmaps=False,
                      annotate=False, jpeg_quality=75, jpeg_subsampling='4:2:0', plot_maps=False, entropy='host',
                      groundtruth=None, flip=False, scales=None, track=None, track_style=None, pose_nms=None, anonymize=None,
                      crops=None, density=None, trails=None, zones=None, track_eval=None):
        """`predict_images` for frames as a camera or a TFRecord holds them: JPEG bytes. The host runs the marker scan and the
        Huffman decode; dequantisation, inverse DCT, chroma upsampling and YCbCr -> RGB run on the device (mpn_jpeg_decode)
        and write the packed source buffer the resize reads - the bytes Pillow decodes, so every result equals
        `predict_images([pillow_decode(j) for j in jpegs], ...)`. Progressive and Adobe CMYK files have every scan
        decoded on the host (mpn_jpeg_scans_decode) and the rest on the device like the others; a stream outside the supported
        set (arithmetic coding, YCCK, ...) is decoded by Pillow and uploaded as pixels, inside the same batch. With entropy='device' the host only parses
        headers: the files' own bytes are uploaded (about a tenth of the coefficients) and the Huffman decode runs on the device
        too (mpn_jpeg_entropy_decode_device); an image it cannot settle takes the host decode. The same results either way.

        Arguments:
            jpegs: a list of b >= 1 `bytes`, one JPEG file each; the image sizes may all differ.
            entropy: 'host' (default) or 'device'. `self.jpeg_staged_bytes` / `self.jpeg_fallbacks`: what the call uploaded for
                the decode, and how many images took the fallback.
            size, keep_aspect_ratio, score_threshold, return_heatmaps, annotate, jpeg_quality, jpeg_subsampling, plot_maps: as
                for `predict_images` (annotate=True draws on the decoded frames; 'jpeg' also encodes them again on the device).
            groundtruth: as for `predict_images` (source pixels).
            flip, scales, track, track_style, pose_nms, track_eval, zones, anonymize: as for `predict_images`.
            crops: as for `predict_images`: cut from the decoded frames (with anonymize= the anonymised ones, never the
                overlays).
        Returns what `predict_images` returns. The decode launches run on the stream ahead of the captured graph, which is the
        one `predict_images` replays: keyed by capacity, not by the batch's sizes.
        """
        def shape():
            if isinstance(jpegs, (bytes, bytearray, memoryview)):
                raise ValueError("jpegs must be a list of bytes (got one bytes object)")
            items = list(jpegs)
            if len(items) < 1:
                raise ValueError("empty batch")
            if any(not isinstance(j, (bytes, bytearray, memoryview)) for j in items):
                raise ValueError("a JPEG must be bytes")
            infos = [jpeg.jpeg_info(j) for j in items]
            height, width = resample.check_size(size)
            return len(items), height, width, items, resample.Plan([(i['height'], i['width']) for i in infos], height, width,
                                                                   keep_aspect_ratio, align=16)
        opts, (_, _, _, items, plan) = self._options(
            shape, score_threshold=score_threshold, return_heatmaps=return_heatmaps, annotate=annotate, jpeg_quality=jpeg_quality,
            jpeg_subsampling=jpeg_subsampling, plot_maps=plot_maps, groundtruth=groundtruth, flip=flip, scales=scales,
            track=track, track_style=track_style, pose_nms=pose_nms, track_eval=track_eval, anonymize=anonymize, zones=zones, trails=trails, density=density, crops=crops)
        entries = [jpeg.prepare(j, entropy, extended=True) for j in items]
        for e, (h, w) in zip(entries, plan.sizes):
            if tuple(e.shape) != (h, w, 3):
                raise ValueError(f"a JPEG decodes to {tuple(e.shape)}, its header says {(h, w, 3)}")

        def decode(ent):
            if ent.jpeg is None:
                ent.jpeg = jpeg.JpegBatchDecoder(self.net.device)
            ent.jpeg.decode(entries, ent.sources, plan.src_offsets, torch.cuda.current_stream(self.net.device))
            self.jpeg_staged_bytes, self.jpeg_fallbacks = ent.jpeg.staged_bytes, ent.jpeg.fallbacks
        return self._predict_sources(plan, decode, opts, groundtruth)

    def _predict_sources(self, plan, put_sources, opts, groundtruth):
        """predict_images and predict_jpegs behind their argument checks. put_sources(ent) queues what brings this batch's
        frames to `ent.sources` where `plan` packs them; around it, in stream order: the descriptors, extents and tables in
        one copy, the frames, the drawing's and the encoder's descriptors, the ground truth, the graph."""
        b = plan.b
        eplan = _encode_plan(plan.sizes, plan.src_offsets, opts.jpeg) if opts.jpeg else None
        ent = self._images_entry(plan, opts, eplan)
        nw = plan.meta_words                                        # this batch's words, not the buffers' capacity
        ent.meta_stage.numpy()[:nw] = plan.meta
        ent.meta[:nw].copy_(ent.meta_stage[:nw], non_blocking=True)
        put_sources(ent)
        if opts.annotate:
            ent.draw.place(plan.sizes, plan.src_offsets)
        if ent.anonymize is not None:
            ent.anonymize.place(plan.sizes, plan.src_offsets)
        if ent.crops is not None:
            ent.crops.place(plan.sizes, plan.src_offsets)
        if eplan:
            self._place_encode(ent, eplan)
        if opts.oks:
            ent.oks.place(groundtruth)
        if ent.track_eval is not None:
            ent.track_eval.place(groundtruth, len(groundtruth), rows=False)
        outs = self._run(ent, lambda: self._device_side_images(ent, opts.thr))
        ent.commit()
        persons = self._finish(ent, outs, b, opts.return_heatmaps)
        if opts.return_heatmaps:
            for p, new_size in zip(persons, plan.new_sizes):
                p['resized_size'] = new_size
        return persons

    def _images_entry(self, plan, opts, eplan):
        """The persistent state of predict_images for one (b, h, w, threshold), one set of options (`_Options.tail`: each an
        entry, and a capacity, of its own) and one CAPACITY (bytes of packed sources, words of descriptors + tables, bytes of
        intermediates, each a power of two): pinned staging, device buffers, the captured graph. A batch that fits the
        capacity of an earlier one replays its graph whatever its mix of sizes; one that exceeds it gets larger buffers and a
        new graph. With annotate the packed RGBA output is sized from the capacity of the sources - it grows with them. eplan
        (annotate='jpeg'): the capacity also covers the encoder's coefficients, streams and workspace."""
        b, h, w = plan.b, plan.height, plan.width
        store = self._graphs if self.use_graph else self._eager_batches
        need = (plan.stage_bytes, plan.meta_words, plan.work_bytes) + (eplan.need if eplan else ())
        base, tail = ('images', b, h, w, opts.thr), opts.tail(b)
        cap_key = (base, self.use_graph) + tail
        cap = self._image_capacity.get(cap_key)
        if cap is None or any(n > c for n, c in zip(need, cap)):
            if cap is not None:
                store.pop(base + (cap,) + tail, None)      # superseded: its buffers and graph are never looked up again
            cap = tuple(resample.capacity_for(max(n, c)) for n, c in zip(need, cap or (0,) * len(need)))
            self._image_capacity[cap_key] = cap
        stage_bytes, meta_words, work_bytes = cap[:3]

        def make():
            dev = self.net.device
            if _lib.lib().mpn_image_resize_desc_bytes() != resample.DESC_WORDS * 4:
                raise _lib.MpnError("mpn_image_resize: the descriptor's layout is not the one this binding was written against")
            return _Entry(stage=torch.zeros(stage_bytes, dtype=torch.uint8).pin_memory(),
                          sources=torch.zeros(stage_bytes, dtype=torch.uint8, device=dev),
                          meta_stage=torch.zeros(meta_words, dtype=torch.int32).pin_memory(),
                          meta=torch.zeros(meta_words, dtype=torch.int32, device=dev),
                          work=torch.empty(work_bytes, dtype=torch.uint8, device=dev))
        return self._entry(opts, base + (cap,), (b, h, w), make, (stage_bytes,) + cap[3:])

    def _device_side_images(self, ent, thr):
        """mpn_image_resize (ragged sources -> the uint8 canvas batch) -> _device_side_batch with mpn_pose_gather_sized last."""
        x, meta = ent.x, ent.meta
        _, h, w, _ = x.shape
        b = ent.tta.b if ent.tta is not None else x.shape[0]
        extent = meta[b * resample.DESC_WORDS:b * (resample.DESC_WORDS + 4)].view(torch.float32).view(b, 4)
        tables = meta[b * (resample.DESC_WORDS + 4):]
        _lib.call("mpn_image_resize", _lib.ptr(ent.sources), _lib.ptr(tables), _lib.ptr(meta), b, h, w, _lib.ptr(x),
                  _lib.ptr(ent.work), ent.work.numel(), _lib.stream_ptr())
        return self._device_side_batch(ent, thr, extent, frames=ent.sources)

    def _assigner_for(self, n):
        a = self._batch_assigners.get(n)
        if a is None:
            from ..prn_inference import KeypointAssigner
            a = self._batch_assigners[n] = KeypointAssigner(self.assigner.net.for_batch(n), self.assigner.threshold)
        return a

    def _has_heatmaps(self):
        """Whether the graph has the keypoint subnet's heatmap head (what plot_maps=True shows)."""
        return getattr(self.net, 'heat_w', None) is not None

    def _variable_versions(self):
        return (self.net.var_version, self.retinanet.var_version if self.retinanet is not None else -1,
                self.assigner.net.var_version if self.assigner is not None else -1)
