"""StackedDenseLayer and ParasiticStackedDenseLayer -- drop-ins for rec_now/layers/stacked_dense_layer.py.

StackedDenseLayer adds resnet_weight times the sum of K per-row parameter rows (B, D*U+U) to the layer's kernel and bias.  It runs on
the same HIP kernel pair as StarDenseLayer (csrc/star_dense.hip) in its additive mode: no (B, D, U) temporary.
"""
from ._ops import STAR_ADD
from ._keras import get_initializer
from .star_dense_layer import ParasiticStarDenseLayer, _PersonalisedDense


class StackedDenseLayer(_PersonalisedDense):
    """Dense layer with per-row parameters: y = act(x . (kernel + w sum_k P_k[:DU]) + bias + w sum_k P_k[DU:]), w = resnet_weight.

    Symbols: B batch size, D input dim, U output dim, K number of parameter tensors (<= 4)."""

    _mode = STAR_ADD

    def __init__(self, units, **kwargs):
        """units: output dim; other kwargs as keras.layers.Dense."""
        super().__init__(units, **kwargs)

    @classmethod
    def get_resnet_param_size(cls, units_in, units_out):
        """Width of one parameter row: D*U + U."""
        return units_in * units_out + units_out

    @classmethod
    def get_resnet_kernel_initializer(cls):
        """Zeros: the per-scene kernel is added to the shared one."""
        return get_initializer('zeros')

    @classmethod
    def get_resnet_bias_initializer(cls):
        """Zeros."""
        return get_initializer('zeros')

    def call(self, inputs, resnet_param_list, resnet_weight=1.0):
        """inputs (B, D); resnet_param_list: a (B, D*U+U) tensor or a list of them; resnet_weight: float.  Returns (B, U)."""
        return self._run(inputs, resnet_param_list, float(resnet_weight))


class ParasiticStackedDenseLayer(ParasiticStarDenseLayer):
    """As ParasiticStarDenseLayer, with kernel = trunk_kernel + parasitic_kernel[g] (the parasitic kernel starts at zeros).

    As in the reference (stacked_dense_layer.py:185-205), only group_idx None leaves the kernel to the trunk: a negative int
    indexes the parasitic kernels from the end, while the bias still takes the trunk alone."""

    def __init__(self, kernel=None, bias=None, dense_layer=None, activation=None, parasitic_kernel_initializer='Zeros', num_groups=1,
                 **kwargs):
        super().__init__(kernel=kernel, bias=bias, dense_layer=dense_layer, activation=activation,
                         parasitic_kernel_initializer=parasitic_kernel_initializer, num_groups=num_groups, **kwargs)

    def _get_kernel(self, group_idx, stop_trunk_grad):
        kernel = self.trunk_kernel.detach() if stop_trunk_grad else self.trunk_kernel
        if group_idx is None:
            return kernel
        return kernel + self.parasitic_kernel[group_idx]
