"""rec_now_amd.layers -- MI355X-native counterparts of rec_now/layers (same module and symbol names)."""
from .multi_hash_layer import FastMultiHashLayer, MultiHashLayer  # noqa: F401
