"""rec_now_amd.layers -- MI355X-native counterparts of rec_now/layers (same module and symbol names)."""
from .afm_layer import AFMLayer  # noqa: F401
from .bilinear_interaction_layer import BilinearInteractionLayer  # noqa: F401
from .can_layer import CANLayer  # noqa: F401
from .cartesian_product_layer import CartesianProductLayer, CrossedIds  # noqa: F401
from .fix_length_layer import FixLengthLayer  # noqa: F401
from .interacting_layer import InteractingLayer  # noqa: F401
from .multi_hash_layer import FastMultiHashLayer, MultiHashLayer  # noqa: F401
from .pooling_layer import PoolingLayer  # noqa: F401
from .target_attention_layer import TargetAttentionLayer  # noqa: F401
