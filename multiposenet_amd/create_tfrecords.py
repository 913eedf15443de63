"""COCO keypoint annotations and images -> TFRecord shards (the reference's data/create_tfrecords.py):

    python -m multiposenet_amd.create_tfrecords --annotations person_keypoints_train2017.json --images train2017 \
        --out records/train [--shards 300 --seed 0 --batch 64]

The masks are made on the device (`coco_records.CocoMaskRasterizer`), a batch of images per call."""
import argparse
import json


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--annotations", required=True, help="COCO person_keypoints_*.json")
    ap.add_argument("--images", required=True, help="directory of the images the JSON names")
    ap.add_argument("--out", required=True, help="directory the shards are written to")
    ap.add_argument("--shards", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0, help="of the image order")
    ap.add_argument("--batch", type=int, default=64, help="images per device call")
    args = ap.parse_args(argv)
    from .coco_records import write_shards
    report = write_shards(args.annotations, args.images, args.out, args.shards, args.seed, args.batch)
    print(f"Number of images: {report['images']}")
    print(f"Number of skipped images: {report['skipped']}")
    print(f"Number of shards: {report['shards']}")
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
