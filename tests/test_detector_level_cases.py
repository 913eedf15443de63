"""Host: the hold-out boxes of tests/detector_level_cases.py reach every detector level. A change of the anchors or of the matching
thresholds fails here, on the CPU, before it silently empties a level of the all-levels gradient test on the GPU."""
import numpy as np

from oracle import retinanet as R

import detector_level_cases as cases


def test_every_level_of_every_image_has_a_matched_anchor():
    anchors, shapes = R.generate_anchors(cases.H, cases.W)
    assert shapes == [(48, 64), (24, 32), (12, 16), (6, 8), (3, 4)]
    boxes, num = cases.boxes_and_num()
    assert boxes.shape == (2, 5, 4) and float(boxes.min()) >= 0.0 and float(boxes.max()) <= 1.0
    for b in range(boxes.shape[0]):
        targets, matches = R.get_training_targets(anchors, boxes[b, :num[b]])
        counts = cases.matched_per_level(matches, shapes, R.NUM_ANCHORS_PER_LOCATION)
        print(f"image {b}: matched anchors per level 3..7 {counts}")
        assert all(c > 0 for c in counts), (b, counts)
        assert counts == cases.MATCHED_PER_LEVEL[b], (b, counts)
        assert set(np.unique(matches[matches >= 0])) == set(range(5))      # every box is somebody's match
        assert np.isfinite(targets).all()
