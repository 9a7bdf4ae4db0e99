"""lzs_compression_amd -- MI355X-native LZS (RFC 1974/2395) block codec.

The product is ``liblzs.so`` (C host + hand-written HIP kernels for gfx950) behind the
reference's one-shot C-ABI (include/lzs/lzs.h); this package is its ctypes front-end plus
the seeded workload generators used by the benchmark and tests.  No CPU codec, no
fallback: without the built library or without a GPU, calls raise.
"""
from .api import (CHANNEL_STATE_BYTES, ChannelCodec, channels_burst_split_work_bytes, channels_burst_work_bytes, compress_channels, compress_channels_burst,
                  decompress_channels, decompress_channels_burst, new_channel_states)
from .api import (IncrementalCompressor, IncrementalDecompressor, LzsError, backend_info, compact, compress, compress_batch, compress_blocks,
                  compress_blocks_sync, compress_stream, compressed_max, decompress, decompress_batch, decompress_blocks, decompress_blocks_sync, decompress_concat,
                  decompress_stream, decompressed_max, incremental_compress, last_error, lib, release_thread_cache)
from .api import (STATUS_END_MARKER, STATUS_ERROR, STATUS_INPUT_FINISHED, STATUS_INPUT_STARVED, STATUS_NO_OUTPUT_BUFFER_SPACE)
from .api import decompress_blocks_dense, decompressed_sizes
from .api import SIZE_CONCAT, decompressed_size, decompressed_size_stream, decompressed_sizes_sync
from .api import decompress_channels_packed, decompress_dense, decompress_packed, decompressed_sizes_packed, offsets_from_sizes
from .api import compact_packed, compress_channels_packed, compress_dense, compress_packed, compressed_bounds_packed
from .api import (channels_burst_packed_split_work_bytes, compress_channels_burst_packed, compress_channels_dense,
                  decompress_channels_burst_packed, decompress_channels_dense)
from .api import PACKET_RESET
from . import workload

__all__ = ["CHANNEL_STATE_BYTES", "ChannelCodec", "channels_burst_split_work_bytes", "channels_burst_work_bytes", "compress_channels", "compress_channels_burst",
           "decompress_channels", "decompress_channels_burst", "new_channel_states",
           "IncrementalCompressor", "IncrementalDecompressor", "LzsError", "backend_info", "compact", "compress", "compress_batch", "compress_blocks",
           "compress_blocks_sync", "compress_stream", "compressed_max", "decompress", "decompress_batch", "decompress_blocks", "decompress_blocks_sync", "decompress_concat",
           "decompress_stream", "decompressed_max", "incremental_compress", "last_error", "lib", "release_thread_cache", "workload",
           "STATUS_END_MARKER", "STATUS_ERROR", "STATUS_INPUT_FINISHED", "STATUS_INPUT_STARVED", "STATUS_NO_OUTPUT_BUFFER_SPACE",
           "decompress_blocks_dense", "decompressed_sizes",
           "SIZE_CONCAT", "decompressed_size", "decompressed_size_stream", "decompressed_sizes_sync",
           "decompress_channels_packed", "decompress_dense", "decompress_packed", "decompressed_sizes_packed", "offsets_from_sizes",
           "compact_packed", "compress_channels_packed", "compress_dense", "compress_packed", "compressed_bounds_packed",
           "channels_burst_packed_split_work_bytes", "compress_channels_burst_packed", "compress_channels_dense",
           "decompress_channels_burst_packed", "decompress_channels_dense",
           "PACKET_RESET"]
