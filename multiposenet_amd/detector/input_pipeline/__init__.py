"""The keypoint input pipeline (reference detector/input_pipeline/): TFRecord reading, host-side sampling of the
augmentations, the on-device augmentation kernel and target-heatmap rendering."""
from .heatmap_creation import get_heatmaps, get_heatmaps_batch, HeatmapRenderer  # noqa: F401
from .tfrecord import read_records, parse_example, decode_keypoint_example  # noqa: F401
from .keypoints_detector_pipeline import KeypointPipeline  # noqa: F401
