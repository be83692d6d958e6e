"""Write an image shard set (kubedl_amd/data/shards.py) for ``resnet50 --data``.

  python scripts/make_image_shards.py OUT --from-npy IMAGES.npy LABELS.npy [--classes L]
  python scripts/make_image_shards.py OUT --synthetic --count 4096 --classes 10 --size 256 --seed 0

``--from-npy`` turns a pair of arrays (uint8 [N, H, W, 3], integer [N]) into a
set.  ``--synthetic`` writes a learnable set with no download: the class picks a
low-frequency colour and orientation pattern, noise is added, so a short job
shows a falling loss.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kubedl_amd.data.shards import synthetic_images, write_shards  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", help="directory of the set")
    ap.add_argument("--from-npy", nargs=2, metavar=("IMAGES", "LABELS"))
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=None, help="default: 10 (synthetic) or max label + 1")
    ap.add_argument("--size", type=int, default=256, help="stored side of the synthetic images")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--shard-size", type=int, default=1024)
    a = ap.parse_args(argv)
    if bool(a.from_npy) == bool(a.synthetic):
        ap.error("give exactly one of --from-npy and --synthetic")
    if a.synthetic:
        classes = a.classes or 10
        images, labels = synthetic_images(a.count, classes, a.size, a.seed)
    else:
        images = np.load(a.from_npy[0], mmap_mode="r", allow_pickle=False)
        labels = np.load(a.from_npy[1], allow_pickle=False)
        classes = a.classes or int(labels.max()) + 1
    meta = write_shards(a.out, images, labels, a.shard_size, classes)
    print(f"{a.out}: {meta['count']} images {meta['height']}x{meta['width']}, {meta['classes']} classes, "
          f"{len(meta['shards'])} shards")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
