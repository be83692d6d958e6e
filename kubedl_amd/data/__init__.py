"""Image input of the PyTorchJob data plane: uint8 shard sets (shards.py), the
host-side order / augmentation plan (plan.py), the resample rule on torch ops
(augment.py) and the per-rank input object (input.py)."""
