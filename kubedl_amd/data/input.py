"""The image input of a rank: ``ShardInput.next(step) -> (x, y)``.

``resident``: the rank's owned partition (image ``i`` of the set belongs to rank
``i % world``) is uploaded once as uint8, with its labels; the epoch's plan
table is uploaded once per epoch; ``next`` is ONE ``augment_batch`` launch
(csrc/augment.hip) with ``row0 = (step % steps_per_epoch) * batch`` -- no host
work per step and no torch kernels.

``stream``: for sets that do not fit in HBM.  A loader thread, backed by a
gather pool of ``workers`` threads, copies the next batches' stored images from
the memory-mapped shards into pinned uint8 buffers (a ring three deep), issues
the host-to-device copy on a copy stream and records an event; ``next`` makes
the compute stream wait on that event and runs the same kernel on the staged
batch with a per-batch plan whose ``src`` is ``0..B-1``.  A pinned buffer is
reused only after its copy event has completed, a device staging buffer only
after the kernel that read it.  The time ``next`` blocks on the loader
accumulates in ``data_wait_ms``; a failure in the loader thread is re-raised in
``next``.

``auto``: ``resident`` when the owned bytes fit the budget (``resident_gb``;
default 25 % of the smaller of the device's free memory and the
``KDL_HBM_LIMIT_GB`` slice where one is set), else ``stream``.

``next`` must be called on the stream the consumer computes on (the trainer's
compute stream): the returned tensors are ordered on it.  Two ``x`` (and ``y``)
buffers alternate.  ResNetEngine.forward_backward joins its weight-gradient side
stream into the compute stream before it returns, so a single buffer would be
safe with today's engine; the second buffer (77 MB at batch 256, 224 px) keeps
the input independent of where that join sits and leaves the previous batch
readable while the next is produced.

On the CPU both modes call ``augment_reference`` (data/augment.py).
"""
from __future__ import annotations

import os
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from kubedl_amd.data.augment import augment_batch, augment_reference, norm_coeffs
from kubedl_amd.data.plan import InputPlan
from kubedl_amd.data.shards import ImageShards

RING = 3
_UPLOAD_CHUNK = 64 << 20  # bytes of stored images per upload step of the resident partition


def resident_budget_bytes(device: torch.device, resident_gb=None) -> int:
    if resident_gb is not None:
        return int(float(resident_gb) * (1 << 30))
    if device.type != "cuda":
        return 1 << 62
    free = torch.cuda.mem_get_info(device)[0]
    lim = os.environ.get("KDL_HBM_LIMIT_GB")
    if lim:
        free = min(free, int(float(lim) * (1 << 30)))
    return free // 4


class _Slot:
    """One stage of the stream ring: pinned host buffers, device staging buffers."""

    def __init__(self, batch: int, H: int, W: int, device: torch.device):
        hip = device.type == "cuda"
        self.images = torch.empty(batch, H, W, 3, dtype=torch.uint8, pin_memory=hip)
        self.labels = torch.empty(batch, dtype=torch.int64, pin_memory=hip)
        self.plan = torch.empty(batch, 8, dtype=torch.int32, pin_memory=hip)
        self.d_images = torch.empty_like(self.images, device=device) if hip else self.images
        self.d_labels = torch.empty_like(self.labels, device=device) if hip else self.labels
        self.d_plan = torch.empty_like(self.plan, device=device) if hip else self.plan
        self.copied = None    # event: this slot's last host-to-device copy
        self.consumed = None  # event: the last kernel that read the device buffers


class ShardInput:
    def __init__(self, shards: ImageShards, info, batch: int, image: int, seed: int = 0, mode: str = "auto",
                 train: bool = True, workers: int = 4, resident_gb=None, max_batches: int = 0):
        if mode not in ("auto", "resident", "stream"):
            raise ValueError(f"ShardInput: mode {mode!r}")
        self.shards = shards
        self.device = torch.device(info.device)
        self.hip = self.device.type == "cuda"
        self.batch, self.OH, self.OW = int(batch), int(image), int(image)
        self.plan = InputPlan(shards.count, shards.height, shards.width, info.world_size, info.rank, batch,
                              seed=seed, train=train)
        self.train = train
        self.steps_per_epoch = self.plan.steps_per_epoch
        self.dropped = self.plan.dropped
        self.max_batches = int(max_batches)
        if self.steps_per_epoch < 1:
            raise ValueError(f"ShardInput: {shards.dir}: {self.plan.n_own} owned images make no full batch of {batch}")
        self.owned_bytes = self.plan.n_own * shards.image_bytes
        if mode == "auto":
            mode = "resident" if self.owned_bytes <= resident_budget_bytes(self.device, resident_gb) else "stream"
        self.mode = mode
        self.A, self.B = norm_coeffs(shards.mean, shards.std)
        self.data_wait_ms = 0.0
        self.plan_uploads = 0
        self.batches = 0
        self._x = [None, None]
        self._y = [None, None]
        self._epoch = None        # epoch of the cached plan table
        self._rows = None         # its host rows
        self._d_rows = None       # its device copy (resident, GPU)
        self.workers = max(int(workers), 1)
        self._thread = None
        self._pool = None
        self._expect = None       # step the loader delivers next
        if mode == "resident":
            self._upload()
        else:
            self._slots = [_Slot(self.batch, shards.height, shards.width, self.device) for _ in range(RING)]
            self._copy_stream = torch.cuda.Stream(self.device) if self.hip else None

    # ------------------------------------------------------------ resident
    def _upload(self) -> None:
        sh, n = self.shards, self.plan.n_own
        self.images = torch.empty(n, sh.height, sh.width, 3, dtype=torch.uint8, device=self.device)
        per = max(1, _UPLOAD_CHUNK // sh.image_bytes)
        for lo in range(0, n, per):
            hi = min(lo + per, n)
            chunk = torch.from_numpy(sh.gather(self.plan.global_index(np.arange(lo, hi))))
            self.images[lo:hi].copy_(chunk)
        self.labels = torch.from_numpy(sh.gather_labels(self.plan.global_index(np.arange(n)))).to(self.device)

    def _epoch_rows(self, e: int) -> np.ndarray:
        if not self.train:
            e = 0  # the eval plan does not depend on the epoch
        if e != self._epoch:
            self._rows = self.plan.epoch(e).rows
            self._epoch = e
            self._d_rows = None
        return self._rows

    def _out(self):
        k = self.batches & 1
        self.batches += 1
        if self._x[k] is None:
            x = torch.empty(self.batch, self.OH, self.OW, 3, dtype=torch.bfloat16, device=self.device)
            self._x[k] = x.permute(0, 3, 1, 2)
            self._y[k] = torch.empty(self.batch, dtype=torch.int64, device=self.device)
        return self._x[k], self._y[k]

    def _next_resident(self, step: int):
        e, r0 = self.plan.locate(step)
        rows = self._epoch_rows(e)
        if not self.hip:
            return augment_reference(self.images, self.labels, torch.from_numpy(rows[r0:r0 + self.batch]),
                                     self.OH, self.OW, self.shards.mean, self.shards.std)
        if self._d_rows is None:
            # once per epoch; from pinned memory, so the host does not wait for the stream to drain
            self._h_rows = torch.from_numpy(rows).pin_memory()
            self._d_rows = self._h_rows.to(self.device, non_blocking=True)
            self.plan_uploads += 1
        x, y = self._out()
        augment_batch(self.images, self.labels, self._d_rows, r0, self.batch, self.OH, self.OW, self.A, self.B, x, y)
        return x, y

    # ------------------------------------------------------------ stream
    def _gather_into(self, slot: _Slot, gidx: np.ndarray) -> None:
        out = slot.images.numpy()
        parts = [p for p in np.array_split(np.arange(len(gidx)), self.workers) if len(p)]
        futs = [self._pool.submit(self.shards.gather, gidx[p], out[p[0]:p[-1] + 1]) for p in parts]
        for f in futs:
            f.result()
        slot.labels.numpy()[:] = self.shards.gather_labels(gidx)

    def _loader(self, step: int, free: "queue.Queue", ready: "queue.Queue", stop: threading.Event) -> None:
        try:
            if self.hip:
                torch.cuda.set_device(self.device)
            epoch, rows = None, None
            while not stop.is_set():
                k = free.get()
                if k is None or stop.is_set():
                    return
                slot = self._slots[k]
                e, r0 = self.plan.locate(step)
                if not self.train:
                    e = 0
                if e != epoch:
                    rows, epoch = self.plan.epoch(e).rows, e
                br = rows[r0:r0 + self.batch]
                if slot.copied is not None:
                    slot.copied.synchronize()  # the pinned buffers are free once their copy is done
                self._gather_into(slot, self.plan.global_index(br[:, 0]))
                p = slot.plan.numpy()
                p[:] = br
                p[:, 0] = np.arange(self.batch)
                if self.hip:
                    with torch.cuda.stream(self._copy_stream):
                        if slot.consumed is not None:
                            self._copy_stream.wait_event(slot.consumed)
                        slot.d_images.copy_(slot.images, non_blocking=True)
                        slot.d_labels.copy_(slot.labels, non_blocking=True)
                        slot.d_plan.copy_(slot.plan, non_blocking=True)
                        slot.copied = torch.cuda.Event()
                        slot.copied.record(self._copy_stream)
                ready.put((step, k))
                step += 1
        except BaseException as e:  # surfaced by next()
            ready.put(e)

    def _start(self, step: int) -> None:
        self._stop()
        self._pool = ThreadPoolExecutor(self.workers, thread_name_prefix="kdl-gather")
        self._free, self._ready, self._stop_evt = queue.Queue(), queue.Queue(), threading.Event()
        for k in range(RING):
            self._free.put(k)
        self._expect = step
        self._thread = threading.Thread(target=self._loader, name="kdl-loader", daemon=True,
                                        args=(step, self._free, self._ready, self._stop_evt))
        self._thread.start()

    def _stop(self) -> None:
        if self._thread is not None:
            self._stop_evt.set()
            self._free.put(None)
            self._thread.join()
            self._thread = None
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        self._expect = None

    def _next_stream(self, step: int):
        if self._thread is None or self._expect != step:
            self._start(step)  # first call, a resume point, or a new pass over an eval set
        t = time.perf_counter()
        item = self._ready.get()
        self.data_wait_ms += (time.perf_counter() - t) * 1e3
        if isinstance(item, BaseException):
            self._stop()
            raise item
        got, k = item
        assert got == step, (got, step)
        self._expect = step + 1
        slot = self._slots[k]
        if not self.hip:
            out = augment_reference(slot.images, slot.labels, slot.plan.clone(), self.OH, self.OW,
                                    self.shards.mean, self.shards.std)
            self._free.put(k)
            return out
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(slot.copied)
        x, y = self._out()
        augment_batch(slot.d_images, slot.d_labels, slot.d_plan, 0, self.batch, self.OH, self.OW, self.A, self.B, x, y)
        slot.consumed = torch.cuda.Event()
        slot.consumed.record(cur)
        self._free.put(k)
        return x, y

    # ------------------------------------------------------------ public
    def next(self, step: int):
        """``(x bf16 [B, 3, OH, OW] channels_last, y int64 [B])`` of step ``step``,
        ordered on the current stream."""
        if self.mode == "resident":
            return self._next_resident(int(step))
        return self._next_stream(int(step))

    def __len__(self) -> int:
        n = self.steps_per_epoch
        return min(n, self.max_batches) if self.max_batches > 0 else n

    def __iter__(self):
        """One pass (an eval set): the batches of steps ``0 .. len-1``."""
        for s in range(len(self)):
            yield self.next(s)

    def close(self) -> None:
        """Stop and join the loader."""
        self._stop()
