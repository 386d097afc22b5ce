from .datasets import (DevicePrefetcher, SyntheticTiles, TileDataset, cat_adjacent,
                       device_random_batch, join_batches, load_files, split_batch, to_tensors)
from .sampler import ShardedSampler
from .scenes import (SceneCropDataset, crop_gather_reference, crop_params_reference,
                     load_scenes, rotation_table, warp_gather_reference, warp_params_reference,
                     zoom_steps)

__all__ = ["SyntheticTiles", "TileDataset", "ShardedSampler", "load_files", "to_tensors",
           "device_random_batch", "split_batch", "cat_adjacent", "join_batches", "DevicePrefetcher",
           "SceneCropDataset", "load_scenes", "crop_params_reference", "crop_gather_reference",
           "zoom_steps", "rotation_table", "warp_params_reference", "warp_gather_reference"]
