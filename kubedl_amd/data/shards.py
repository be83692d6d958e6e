"""Image shard sets: a directory of uint8 image arrays with a ``meta.json``.

    {"version": 1, "count": N, "height": H, "width": W, "channels": 3, "classes": L,
     "mean": [r, g, b], "std": [r, g, b],
     "shards": [{"images": "images-00000.npy", "labels": "labels-00000.npy", "count": n}]}

``images-*.npy`` is ``uint8 [n, H, W, 3]`` in C order, ``labels-*.npy`` is
``int64 [n]``.  ``mean`` / ``std`` are in 0..255 units and optional (default:
the ImageNet values times 255).  All images of a set share one stored size:
decoding and coarse resizing happen offline (for 224 px training store about
256 px).  Files are opened with ``numpy.load(mmap_mode="r", allow_pickle=False)``:
no pickle, nothing in a set is executed.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence

import numpy as np

VERSION = 1
IMAGENET_MEAN = (0.485 * 255.0, 0.456 * 255.0, 0.406 * 255.0)
IMAGENET_STD = (0.229 * 255.0, 0.224 * 255.0, 0.225 * 255.0)


def _fail(path: str, why: str):
    raise ValueError(f"{path}: {why}")


class ImageShards:
    """A validated, memory-mapped shard set.  ``images[k]`` / ``labels[k]`` are the
    k-th shard's arrays; ``gather(idx)`` copies images by global index."""

    def __init__(self, directory: str, meta: dict, images: List[np.ndarray], labels: List[np.ndarray]):
        self.dir = directory
        self.meta = meta
        self.images = images
        self.labels = labels
        self.count = int(meta["count"])
        self.height = int(meta["height"])
        self.width = int(meta["width"])
        self.classes = int(meta["classes"])
        self.mean = tuple(float(v) for v in meta.get("mean", IMAGENET_MEAN))
        self.std = tuple(float(v) for v in meta.get("std", IMAGENET_STD))
        self._starts = np.cumsum([0] + [a.shape[0] for a in images])  # shard k holds [starts[k], starts[k+1])

    @classmethod
    def open(cls, directory: str) -> "ImageShards":
        mpath = os.path.join(directory, "meta.json")
        try:
            with open(mpath) as f:
                meta = json.load(f)
        except (OSError, ValueError) as e:
            _fail(mpath, f"cannot read ({e})")
        if not isinstance(meta, dict):
            _fail(mpath, "not a JSON object")
        if meta.get("version") != VERSION:
            _fail(mpath, f"version {meta.get('version')!r}, this reader knows version {VERSION}")
        for k in ("count", "height", "width", "channels", "classes"):
            if not isinstance(meta.get(k), int) or isinstance(meta.get(k), bool) or meta[k] < (0 if k == "count" else 1):
                _fail(mpath, f"{k!r} must be a positive integer, got {meta.get(k)!r}")
        if meta["channels"] != 3:
            _fail(mpath, f"channels {meta['channels']}, only 3 is supported")
        for k in ("mean", "std"):
            if k in meta:
                v = meta[k]
                if not (isinstance(v, list) and len(v) == 3 and all(isinstance(t, (int, float)) for t in v)):
                    _fail(mpath, f"{k!r} must be three numbers")
                if k == "std" and not all(t > 0 for t in v):
                    _fail(mpath, "'std' must be positive")
        shards = meta.get("shards")
        if not isinstance(shards, list) or not all(isinstance(s, dict) for s in shards):
            _fail(mpath, "'shards' must be a list of objects")
        total = sum(int(s.get("count", -1)) for s in shards)
        if total != meta["count"]:
            _fail(mpath, f"shard counts sum to {total}, 'count' says {meta['count']}")
        H, W, L = meta["height"], meta["width"], meta["classes"]
        images, labels = [], []
        for s in shards:
            n = int(s["count"])
            arrs = []
            for key in ("images", "labels"):
                name = s.get(key)
                if not isinstance(name, str) or os.path.basename(name) != name:
                    _fail(mpath, f"shard {key!r} must be a plain file name, got {name!r}")
                path = os.path.join(directory, name)
                try:
                    arrs.append((path, np.load(path, mmap_mode="r", allow_pickle=False)))
                except (OSError, ValueError) as e:
                    _fail(path, f"cannot open ({e})")
            (ipath, img), (lpath, lab) = arrs
            if img.dtype != np.uint8:
                _fail(ipath, f"dtype {img.dtype}, expected uint8")
            if img.shape != (n, H, W, 3) or not img.flags["C_CONTIGUOUS"]:
                _fail(ipath, f"shape {img.shape}, expected {(n, H, W, 3)} in C order")
            if lab.dtype != np.int64:
                _fail(lpath, f"dtype {lab.dtype}, expected int64")
            if lab.shape != (n,):
                _fail(lpath, f"shape {lab.shape}, expected {(n,)}")
            if n and (int(lab.min()) < 0 or int(lab.max()) >= L):
                _fail(lpath, f"labels span [{int(lab.min())}, {int(lab.max())}], outside [0, {L})")
            images.append(img)
            labels.append(lab)
        return cls(directory, meta, images, labels)

    @property
    def image_bytes(self) -> int:
        return self.height * self.width * 3

    def gather(self, idx: Sequence[int], out: Optional[np.ndarray] = None) -> np.ndarray:
        """Copy the images with global indices ``idx`` into ``out`` ([len, H, W, 3] uint8)."""
        idx = np.asarray(idx, dtype=np.int64)
        if out is None:
            out = np.empty((len(idx), self.height, self.width, 3), np.uint8)
        if len(idx) and (idx.min() < 0 or idx.max() >= self.count):
            raise IndexError(f"{self.dir}: image index outside [0, {self.count})")
        shard = np.searchsorted(self._starts, idx, side="right") - 1
        for j, (k, i) in enumerate(zip(shard, idx)):
            out[j] = self.images[k][i - self._starts[k]]
        return out

    def gather_labels(self, idx: Sequence[int]) -> np.ndarray:
        idx = np.asarray(idx, dtype=np.int64)
        shard = np.searchsorted(self._starts, idx, side="right") - 1
        return np.array([self.labels[k][i - self._starts[k]] for k, i in zip(shard, idx)], dtype=np.int64)


def _save_npy(path: str, arr: np.ndarray) -> None:
    tmp = path + f".tmp{os.getpid()}"
    with open(tmp, "wb") as f:
        np.save(f, arr, allow_pickle=False)
    os.replace(tmp, path)


def write_shards(directory: str, images, labels, shard_size: int, classes: int, mean=None, std=None) -> dict:
    """Write ``images`` (uint8 [N, H, W, 3]) / ``labels`` (int [N]) as a set of
    shards of ``shard_size`` images (the last one may be shorter).  Every file is
    written to a temporary name and renamed; ``meta.json`` goes last, so a set
    with a ``meta.json`` is complete."""
    images = np.asarray(images)
    labels = np.asarray(labels)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
        raise ValueError(f"write_shards: images must be uint8 [N, H, W, 3], got {images.dtype} {images.shape}")
    if labels.shape != (images.shape[0],) or labels.dtype.kind not in "iu":
        raise ValueError(f"write_shards: labels must be integers [N], got {labels.dtype} {labels.shape}")
    labels = labels.astype(np.int64)
    if len(labels) and (labels.min() < 0 or labels.max() >= classes):
        raise ValueError(f"write_shards: labels outside [0, {classes})")
    if shard_size < 1:
        raise ValueError("write_shards: shard_size >= 1")
    os.makedirs(directory, exist_ok=True)
    N, H, W, _ = images.shape
    shards = []
    for k, lo in enumerate(range(0, N, shard_size)):
        hi = min(lo + shard_size, N)
        names = {"images": f"images-{k:05d}.npy", "labels": f"labels-{k:05d}.npy"}
        _save_npy(os.path.join(directory, names["images"]), np.ascontiguousarray(images[lo:hi]))
        _save_npy(os.path.join(directory, names["labels"]), np.ascontiguousarray(labels[lo:hi]))
        shards.append({**names, "count": hi - lo})
    meta = {"version": VERSION, "count": int(N), "height": int(H), "width": int(W), "channels": 3,
            "classes": int(classes)}
    if mean is not None:
        meta["mean"] = [float(v) for v in mean]
    if std is not None:
        meta["std"] = [float(v) for v in std]
    meta["shards"] = shards
    mpath = os.path.join(directory, "meta.json")
    tmp = mpath + f".tmp{os.getpid()}"
    with open(tmp, "w") as f:
        json.dump(meta, f, indent=1)
    os.replace(tmp, mpath)
    return meta


def synthetic_images(count: int, classes: int, size: int, seed: int):
    """A learnable synthetic set: the class picks a low-frequency colour and
    orientation pattern (a sinusoidal grating whose angle, period and colour
    depend on the class), plus uniform noise.  Returns (uint8 [count, size, size, 3],
    int64 [count])."""
    rng = np.random.Generator(np.random.PCG64([int(seed), 7]))
    labels = rng.integers(0, classes, size=count, dtype=np.int64)
    yy, xx = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    images = np.empty((count, size, size, 3), np.uint8)
    for i, c in enumerate(labels):
        ang = np.pi * (int(c) % 8) / 8.0
        period = size / (1.5 + (int(c) // 8) % 4)
        phase = rng.uniform(0, 2 * np.pi)
        wave = np.sin(2 * np.pi * (np.cos(ang) * xx + np.sin(ang) * yy) / period + phase)
        hue = 2 * np.pi * int(c) / max(classes, 1)
        base = 128.0 + 70.0 * np.array([np.cos(hue), np.cos(hue + 2.1), np.cos(hue + 4.2)], np.float32)
        img = base[None, None, :] + 45.0 * wave[:, :, None] + rng.uniform(-25, 25, size=(size, size, 3))
        images[i] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return images, labels
