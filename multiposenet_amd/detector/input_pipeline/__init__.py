"""The input pipelines (reference detector/input_pipeline/): TFRecord reading, host-side sampling of the augmentations, the
on-device augmentation kernel and target-heatmap rendering of the keypoint path, the PRN's crops and labels, and the person
detector's augmentation and boxes."""
from .heatmap_creation import get_heatmaps, get_heatmaps_batch, HeatmapRenderer  # noqa: F401
from .tfrecord import read_records, parse_example, decode_keypoint_example, jpeg_shape  # noqa: F401
from .keypoints_detector_pipeline import KeypointPipeline  # noqa: F401
from .prn_pipeline import PoseResidualNetworkPipeline, AnnotationCache  # noqa: F401
from .person_detector_pipeline import DetectorPipeline  # noqa: F401
