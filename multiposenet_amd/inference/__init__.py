from .utils import get_keypoints, get_keypoints_batch, KeypointDecoder, draw_everything, draw_tracks  # noqa: F401
from .detector import Detector  # noqa: F401
from .draw import TrackStyle  # noqa: F401
from .anonymize_stage import Anonymize, Anonymizer, anonymize  # noqa: F401
from .crops import PersonCrops, PersonCropper, person_crops  # noqa: F401
from .jpeg import JpegBatchEncoder, encode_jpegs  # noqa: F401
from .maps import MapPlotter, plot_maps  # noqa: F401
from ..tracking import PoseTracker, OneEuro, ConstantVelocity  # noqa: F401
from ..pose_nms import PoseNms, PoseSuppressor, pose_nms  # noqa: F401
from ..track_metrics import TrackEvaluator, groundtruth_from_posetrack  # noqa: F401
from ..zones import ZoneCounter  # noqa: F401
from ..trails import TrackTrails, draw_trails  # noqa: F401
from ..density import DensityMap, draw_density  # noqa: F401
