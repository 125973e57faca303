"""myscaledb_amd -- MI355X-native brute-force vector-scan path for MyScaleDB.

The product is libmqvs.so (HIP kernels for gfx950 + the C-ABI in
include/mqvs.h).  This package is its Python-side mirror of the reference
operator surface (vector_scan) plus the multi-GPU row-range sharding
(sharded).  Importing it loads libmqvs.so and fails loudly if it is missing.
"""
from . import _lib  # noqa: F401  (loads libmqvs.so, raises if absent)
from .vector_scan import (  # noqa: F401
    BinaryVectorScanSegment,
    VectorScanSegment,
    binary_batch,
    init,
    merge_shards,
    pack_bitmap,
    set_binary_batch,
    try_brute_force_search,
    try_brute_force_search_binary,
    vector_scan_without_index,
)
from .vector_index import BinaryVectorIndex, VectorIndex, index_blob_info  # noqa: F401
from .part_group import (BinaryPartGroup, PartGroup, part_group_batch, set_part_group_batch,  # noqa: F401
                         set_part_group_binary_rows, set_part_group_rows)
from .index_group import BinaryIndexGroup  # noqa: F401

__all__ = ["PartGroup", "BinaryPartGroup", "BinaryIndexGroup", "set_part_group_binary_rows", "set_part_group_rows", "set_part_group_batch", "part_group_batch", "set_binary_batch", "binary_batch", "index_blob_info","BinaryVectorScanSegment", "try_brute_force_search_binary", "VectorScanSegment", "init", "merge_shards", "pack_bitmap",
           "try_brute_force_search", "vector_scan_without_index", "VectorIndex", "BinaryVectorIndex"]
