"""Generate golden numbers for the detector metrics by running the REFERENCE implementation (`metrics.py`: `Evaluator`,
`evaluate_detector`) on the cases of `metrics_cases.py`.

The reference module is loaded by file path with an empty stand-in registered for `tensorflow.compat.v1` (the module
imports it at the top; `add_groundtruth`, `add_detections` and `evaluate` never touch it). Nothing from it is copied into
this repository - only the seven numbers it returns per case are stored, as float64 in METRIC order, in
`tests/golden/metrics_goldens.npz`.

Run where a checkout of the reference exists:
    MPN_REFERENCE=/path/to/reference PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_metrics_goldens.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics_goldens.npz")
METRICS = ("AP", "precision", "recall", "mean_iou_for_TP", "best_threshold", "total_FP", "total_FN")


def load_reference():
    ref = os.environ.get("MPN_REFERENCE")
    if not ref:
        raise SystemExit("set MPN_REFERENCE to a checkout of the reference project")
    sys.dont_write_bytecode = True
    for name in ("tensorflow", "tensorflow.compat", "tensorflow.compat.v1"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("_ref_metrics", os.path.join(ref, "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


from metrics_cases import cases  # noqa: E402


def main():
    ref = load_reference()
    out, names = {}, []
    for name, images, iou_threshold in cases():
        ev = ref.Evaluator()
        for i, (gt, boxes, scores) in enumerate(images):
            ev.add_groundtruth(str(i), gt)
            ev.add_detections(str(i), boxes, scores)
        ev.evaluate(iou_threshold)
        out[name] = np.array([ev.metrics[m] for m in METRICS], np.float64)
        names.append(name)
        print(name, out[name])
    out["names"] = np.array(names)
    out["metrics"] = np.array(METRICS)
    out["versions"] = np.array([np.__version__])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(names), "cases", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
