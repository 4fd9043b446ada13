"""StarDenseLayer and ParasiticStarDenseLayer -- drop-ins for rec_now/layers/star_dense_layer.py (STAR, arXiv 2101.11427).

StarDenseLayer multiplies the layer's kernel by K per-row parameter rows (B, D*U+U) and adds their bias parts.  The reference forms a
(B, D, U) kernel for that (star_dense_layer.py:140-142); here one HIP kernel pair (csrc/star_dense.hip) reads each parameter row once
and forms the personalised kernel in registers, so the layer keeps no B-times-larger temporary for the forward or the backward.
"""
import torch

from ._keras import DenseBase, Layer, activation_code, get_initializer
from ._ops import STAR_MUL, multi_dense, star_dense
from ..util.param_normalizer import wrap_as_list


class _PersonalisedDense(DenseBase):
    """keras.layers.Dense with per-row parameter rows: `kernel` (D, U), `bias` (U,); call(inputs (B, D), param_list)."""

    _mode = None

    def build(self, input_shape):
        """Creates `kernel` (D, U) and, with use_bias, `bias` (U,) -- the variable names and shapes of keras.layers.Dense."""
        width = input_shape[-1]
        if width is None:
            raise ValueError('The last dimension of the inputs to `Dense` should be defined. Found `None`.')
        self.units_in = int(width)
        self.kernel = self.add_weight('kernel', shape=[self.units_in, self.units], initializer=self.kernel_initializer,
                                      regularizer=self.kernel_regularizer, constraint=self.kernel_constraint)
        self.bias = None
        if self.use_bias:
            self.bias = self.add_weight('bias', shape=[self.units], initializer=self.bias_initializer,
                                        regularizer=self.bias_regularizer, constraint=self.bias_constraint)
        self.built = True

    def _run(self, inputs, param_list, weight):
        if inputs.dim() != 2:
            raise ValueError('%s expects a (B, D) input, got shape %s' % (type(self).__name__, tuple(inputs.shape)))
        D, U = self.units_in, self.units
        if inputs.shape[1] != D:
            raise ValueError('Matrix size-incompatible: In[0]: %s, In[1]: %s' % (list(inputs.shape), [D, U]))
        params = wrap_as_list(param_list)
        if len(params) < 1:
            raise ValueError('%s needs at least one parameter tensor' % type(self).__name__)
        for p in params:
            if p.dim() != 2 or p.shape[1] != D * U + U or p.shape[0] != inputs.shape[0]:
                raise ValueError('each parameter tensor must be (B, D*U+U) = (%d, %d), got %s'
                                 % (inputs.shape[0], D * U + U, tuple(p.shape)))
        out = star_dense(inputs, self.kernel, self.bias, params, self._mode, weight, self.act_code if self.act_code is not None else 0)
        if self.act_callable is not None:
            out = self.act_callable(out)
        return out


class StarDenseLayer(_PersonalisedDense):
    """STAR topology fully-connected layer: y = act(x . (kernel * prod_k P_k[:DU]) + sum_k P_k[DU:] + bias - K).

    Symbols: B batch size, D input dim, U output dim, K number of parameter tensors.  The parameter rows usually come from a table
    indexed by scene: `table[scene]` with the table initialised by get_starnet_kernel_initializer() (ones).  The `- K` is the
    reference's: kernel and bias parts share that ones-initialised table (star_dense_layer.py:152-155)."""

    _mode = STAR_MUL

    def __init__(self, units, **kwargs):
        """units: output dim; other kwargs as keras.layers.Dense."""
        super().__init__(units, **kwargs)

    @classmethod
    def get_starnet_param_size(cls, units_in, units_out):
        """Width of one parameter row (the embedding dim of the table that produces them): D*U + U."""
        return units_in * units_out + units_out

    @classmethod
    def get_starnet_kernel_initializer(cls):
        """Ones: the per-scene kernel multiplies the shared one."""
        return get_initializer('ones')

    @classmethod
    def get_starnet_bias_initializer(cls):
        """Zeros."""
        return get_initializer('zeros')

    def call(self, inputs, starnet_param_list):
        """inputs (B, D); starnet_param_list: a (B, D*U+U) tensor or a list of K <= 4 of them.  Returns (B, U)."""
        return self._run(inputs, starnet_param_list, 1.0)


def _as_initializer(identifier):
    return get_initializer(identifier.lower() if isinstance(identifier, str) else identifier)


class ParasiticStarDenseLayer(Layer):
    """A group of parasitic kernels and biases on an existing dense layer: kernel = trunk_kernel * parasitic_kernel[g],
    bias = trunk_bias + parasitic_bias[g].  One scalar group per call, so the combined (D, U) kernel is formed once and the
    product runs on the MultiDense GEMM (N = 1).

    The trunk is given as `kernel` (D, U) / `bias` (U,) tensors, or as `dense_layer`: any object with `.kernel` / `.bias`
    (and, when it is not built yet, `build(input_shape)`)."""

    def __init__(self, kernel=None, bias=None, dense_layer=None, activation=None, parasitic_kernel_initializer='Ones', num_groups=1,
                 **kwargs):
        super().__init__(**kwargs)
        if dense_layer is not None:
            self.dense_layer = dense_layer
            if getattr(dense_layer, 'built', True):
                self.trunk_kernel, self.trunk_bias = dense_layer.kernel, getattr(dense_layer, 'bias', None)
        else:
            if kernel is None:
                raise ValueError('kernel is None')
            self.dense_layer = None
            self.trunk_kernel, self.trunk_bias = kernel, bias
        self.parasitic_kernel_initializer = parasitic_kernel_initializer
        self.activation = activation
        self.act_code, self.act_callable = activation_code(activation)
        self.num_groups = int(num_groups)

    def _build_dense_layer(self, input_shape):
        if hasattr(self, 'trunk_kernel'):
            return
        if not getattr(self.dense_layer, 'built', True):
            self.dense_layer.build(input_shape)
        self.trunk_kernel, self.trunk_bias = self.dense_layer.kernel, getattr(self.dense_layer, 'bias', None)

    def build(self, input_shape):
        """Creates `kernel` (num_groups, D, U) and, when the trunk has a bias, `bias` (num_groups, U)."""
        self._build_dense_layer(input_shape)
        tk = self.trunk_kernel
        if tk.dim() != 2:
            raise ValueError('the trunk kernel must be (D, U), got shape %s' % (tuple(tk.shape),))
        self._build_device = tk.device
        self.parasitic_kernel = self.add_weight('kernel', shape=[self.num_groups] + list(tk.shape),
                                                initializer=_as_initializer(self.parasitic_kernel_initializer))
        self.parasitic_bias = None
        if self.trunk_bias is not None:
            self.parasitic_bias = self.add_weight('bias', shape=[self.num_groups] + list(self.trunk_bias.shape), initializer='zeros')
        self.built = True

    @staticmethod
    def _only_use_trunk(group_idx):
        return group_idx is None or (isinstance(group_idx, int) and group_idx < 0)

    def _combine_kernel(self, kernel, group_idx):
        return kernel * self.parasitic_kernel[group_idx]

    def _get_kernel(self, group_idx, stop_trunk_grad):
        kernel = self.trunk_kernel.detach() if stop_trunk_grad else self.trunk_kernel
        if self._only_use_trunk(group_idx):
            return kernel
        return self._combine_kernel(kernel, group_idx)

    def _get_bias(self, group_idx, stop_trunk_grad):
        bias = self.trunk_bias
        if bias is None:
            return None
        if stop_trunk_grad:
            bias = bias.detach()
        if self._only_use_trunk(group_idx):
            return bias
        return bias + self.parasitic_bias[group_idx]

    def call(self, inputs, group_idx=0, stop_trunk_grad=False):
        """inputs (B, D); group_idx: int, 0-d integer tensor, or None / a negative int for the trunk alone.  Returns (B, U)."""
        if inputs.dim() != 2:
            raise ValueError('%s expects a (B, D) input, got shape %s' % (type(self).__name__, tuple(inputs.shape)))
        if isinstance(group_idx, torch.Tensor):
            if group_idx.dim() != 0 or group_idx.dtype.is_floating_point:
                raise ValueError('group_idx must be an int or a 0-d integer tensor, got %s' % (group_idx,))
            group_idx = group_idx.to(self.parasitic_kernel.device)
        kernel = self._get_kernel(group_idx, stop_trunk_grad)
        bias = self._get_bias(group_idx, stop_trunk_grad)
        D, U = kernel.shape
        if inputs.shape[1] != D:
            raise ValueError('Matrix size-incompatible: In[0]: %s, In[1]: %s' % (list(inputs.shape), [D, U]))
        out = multi_dense(inputs, kernel.reshape(1, D, U), bias.reshape(1, 1, U) if bias is not None else None,
                          self.act_code if self.act_code is not None else 0)[0]
        if self.act_callable is not None:
            out = self.act_callable(out)
        return out
