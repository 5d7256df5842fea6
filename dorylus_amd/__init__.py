"""dorylus_amd -- MI355X-native aggregation + transform engine behind the
reference's Engine / ResourceComm boundary (see include/dorylus_hip.h).

Only the hot path lives here: HIP kernels + C-ABI (csrc/), the C++ host mirror of
the reference's Engine stages and file formats (host/), and this thin ctypes layer.
"""
from ._lib import (BACKWARD, FORWARD, GAT, GATMH, GCN, LIB_PATH, SYMBOLS, Context,  # noqa: F401
                   DoryError, gatmh_row_gather_bf16_wide_form, halo_send_map, k1_bf16_wide_form, load, option_check, option_specs, row_chunk_plan, row_edge_split_plan, row_interior_plan)
from .engine import Chunk, Engine, NativeEngine  # noqa: F401
from .partition import Partition, read_features, read_labels, read_layer_config  # noqa: F401
