"""The yardstick of the keypoint-AP tests: a plain-loop numpy transcription of pycocotools' COCOeval for
iouType='keypoints' (cocoeval.py: computeOks, evaluateImg, accumulate, summarize), one category, maxDets = [20]. pycocotools
itself is not a dependency of this project. Written independently of multiposenet_amd/pose_metrics.py: it shares no code
with it, keeps COCOeval's loops as loops, and is anchored by closed-form cases in tests/test_pose_eval_host.py.

Detections of an image: a dict with 'scores' f32 [n], 'keypoint_scores' f32 [n,17], 'keypoints' f32 [n,17,3] (x, y, score).
Ground truth of an image: 'keypoints' [g,17,3] (x, y, v), 'boxes' [g,4] (x, y, w, h), optional 'area' [g], 'iscrowd' [g]."""
import numpy as np

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]           # all, medium, large
MAX_DETS = 20
NAMES = ('AP', 'AP50', 'AP75', 'APM', 'APL', 'AR', 'AR50', 'AR75', 'ARM', 'ARL')


def detection_scores(det, score_mode):
    """float32 [n]: mode 0 the box score; mode 1 box score * (keypoint scores summed in order, in float32) / 17."""
    s = np.asarray(det['scores'], np.float32)
    if score_mode == 0:
        return s.copy()
    out = np.zeros(len(s), np.float32)
    for i in range(len(s)):
        m = np.float32(0)
        for k in range(17):
            m = np.float32(m + np.float32(det['keypoint_scores'][i][k]))
        out[i] = np.float32(s[i] * np.float32(m / np.float32(17)))
    return out


def _gt_list(gt):
    """COCOeval._prepare: the image's annotations with 'ignore' = iscrowd or num_keypoints == 0."""
    kp = np.asarray(gt['keypoints'], np.float64).reshape(-1, 17, 3)
    boxes = np.asarray(gt['boxes'], np.float64).reshape(-1, 4)
    anns = []
    for j in range(len(kp)):
        area = float(gt['area'][j]) if gt.get('area') is not None else float(boxes[j][2] * boxes[j][3])
        crowd = int(gt['iscrowd'][j]) if gt.get('iscrowd') is not None else 0
        num_keypoints = int(np.count_nonzero(kp[j][:, 2] > 0))
        anns.append({'keypoints': kp[j].reshape(-1), 'bbox': boxes[j], 'area': area, 'iscrowd': crowd,
                     'ignore': bool(crowd) or num_keypoints == 0, 'index': j})
    return anns


def _dt_list(det, score_mode):
    """COCO.loadRes for keypoints: area = the keypoints' bounding box."""
    scores = detection_scores(det, score_mode)
    dts = []
    for i in range(len(scores)):
        s = np.asarray(det['keypoints'][i], np.float64).reshape(-1)
        x, y = s[0::3], s[1::3]
        x0, x1, y0, y1 = np.min(x), np.max(x), np.min(y), np.max(y)
        dts.append({'keypoints': s, 'score': scores[i], 'area': (x1 - x0) * (y1 - y0), 'index': i})
    return dts


def compute_oks(gts, dts):
    """COCOeval.computeOks: dts already sorted and cut; [len(dts), len(gts)]."""
    ious = np.zeros((len(dts), len(gts)))
    vars_ = (SIGMAS * 2) ** 2
    k = len(SIGMAS)
    for j, gt in enumerate(gts):
        g = np.array(gt['keypoints'])
        xg, yg, vg = g[0::3], g[1::3], g[2::3]
        k1 = np.count_nonzero(vg > 0)
        bb = gt['bbox']
        x0, x1 = bb[0] - bb[2], bb[0] + bb[2] * 2
        y0, y1 = bb[1] - bb[3], bb[1] + bb[3] * 2
        for i, dt in enumerate(dts):
            d = np.array(dt['keypoints'])
            xd, yd = d[0::3], d[1::3]
            if k1 > 0:
                dx, dy = xd - xg, yd - yg
            else:
                z = np.zeros((k))
                dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
            e = (dx ** 2 + dy ** 2) / vars_ / (gt['area'] + np.spacing(1)) / 2
            if k1 > 0:
                e = e[vg > 0]
            total = 0.0
            for v in e:                                               # (np.sum in COCOeval; a plain loop here)
                total += np.exp(-v)
            ious[i, j] = total / e.shape[0]
    return ious


def evaluate_image(det, gt, score_mode=0, max_dets=MAX_DETS):
    """COCOeval.evaluateImg for the three area ranges, in the layout of mpn_oks_match's result: 'rank' int32 [n] (the place
    in the stable descending score order), 'score' f32 [n], 'area' f64 [n], 'matches' int32 [n,3,10] (ground-truth index in
    the image's own order, -1 = none or not evaluated), 'ignore' bool [n,3,10], 'oks' f64 [n, g] (zero rows where not
    evaluated), 'gt_ignore' bool [3, g]."""
    gts, dts_all = _gt_list(gt), _dt_list(det, score_mode)
    n, ng, nt = len(dts_all), len(gts), len(IOU_THRS)
    inds = np.argsort([-d['score'] for d in dts_all], kind='mergesort')
    rank = np.zeros(n, np.int32)
    for place, i in enumerate(inds):
        rank[i] = place
    dts = [dts_all[i] for i in inds[0:max_dets]]
    ious_all = compute_oks(gts, dts)
    out = {'rank': rank, 'score': np.array([d['score'] for d in dts_all], np.float32),
           'area': np.array([d['area'] for d in dts_all], np.float64), 'matches': -np.ones((n, 3, nt), np.int32),
           'ignore': np.zeros((n, 3, nt), bool), 'oks': np.zeros((n, ng)), 'gt_ignore': np.zeros((3, ng), bool)}
    for di, d in enumerate(dts):
        out['oks'][d['index']] = ious_all[di]
    for a, rng in enumerate(AREA_RNG):
        for g in gts:
            g['_ignore'] = 1 if (g['ignore'] or (g['area'] < rng[0] or g['area'] > rng[1])) else 0
        out['gt_ignore'][a] = [g['_ignore'] for g in gts]
        gtind = np.argsort([g['_ignore'] for g in gts], kind='mergesort')
        gs = [gts[i] for i in gtind]
        iscrowd = [int(o['iscrowd']) for o in gs]
        ious = ious_all[:, gtind] if len(ious_all) > 0 else ious_all
        gtm = np.zeros((nt, len(gs)))
        dtm = -np.ones((nt, len(dts)), np.int64)
        gt_ig = np.array([g['_ignore'] for g in gs])
        dt_ig = np.zeros((nt, len(dts)))
        if not len(ious) == 0:
            for tind, t in enumerate(IOU_THRS):
                for dind, d in enumerate(dts):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gs):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = gs[m]['index']
                    gtm[tind, m] = 1
        outside = np.array([d['area'] < rng[0] or d['area'] > rng[1] for d in dts]).reshape((1, len(dts)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == -1, np.repeat(outside, nt, 0)))
        for dind, d in enumerate(dts):
            out['matches'][d['index'], a] = dtm[:, dind]
            out['ignore'][d['index'], a] = dt_ig[:, dind]
    return out


def accumulate(images, max_dets=MAX_DETS):
    """COCOeval.accumulate: images = a list of evaluate_image results -> precision [T, R, 3], recall [T, 3]."""
    nt, nr, na = len(IOU_THRS), len(REC_THRS), len(AREA_RNG)
    precision = -np.ones((nt, nr, na))
    recall = -np.ones((nt, na))
    for a in range(na):
        scores, dtm, dt_ig, gt_ig = [], [], [], []
        for e in images:
            order = [i for i in np.argsort(e['rank'], kind='mergesort') if e['rank'][i] < max_dets]
            scores.extend(e['score'][i] for i in order)
            dtm.extend(e['matches'][i, a] >= 0 for i in order)
            dt_ig.extend(e['ignore'][i, a] for i in order)
            gt_ig.extend(e['gt_ignore'][a])
        npig = np.count_nonzero(np.array(gt_ig) == 0)
        if npig == 0:
            continue
        scores = np.array(scores, np.float32)
        inds = np.argsort(-scores, kind='mergesort')
        dtm = np.array(dtm, bool).reshape(-1, nt).T[:, inds]
        dt_ig = np.array(dt_ig, bool).reshape(-1, nt).T[:, inds]
        tps = np.logical_and(dtm, np.logical_not(dt_ig))
        fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
        tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
        fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
        for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
            tp, fp = np.array(tp), np.array(fp)
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            q = np.zeros((nr,))
            recall[t, a] = rc[-1] if nd else 0
            pr = pr.tolist()
            q = q.tolist()
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            inds_r = np.searchsorted(rc, REC_THRS, side='left')
            try:
                for ri, pi in enumerate(inds_r):
                    q[ri] = pr[pi]
            except IndexError:
                pass
            precision[t, :, a] = np.array(q)
    return precision, recall


def summarize(precision, recall):
    """COCOeval.summarize's _summarizeKps -> the ten numbers by name."""
    def _summarize(ap, iou_thr=None, a=0):
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[..., a]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    stats = [_summarize(1), _summarize(1, .5), _summarize(1, .75), _summarize(1, a=1), _summarize(1, a=2),
             _summarize(0), _summarize(0, .5), _summarize(0, .75), _summarize(0, a=1), _summarize(0, a=2)]
    return dict(zip(NAMES, stats))


def evaluate(dets, gts, score_mode=0, max_dets=MAX_DETS):
    """The ten numbers for lists of per-image detections and ground truth."""
    images = [evaluate_image(d, g, score_mode, max_dets) for d, g in zip(dets, gts)]
    return summarize(*accumulate(images, max_dets))
