"""TargetAttentionLayer -- masked multi-head softmax target attention of a padded behaviour sequence against the candidate item (the
attention of BST, of the softmax variants of DIN and of MHTA pooling); the reference package has no such layer, this module is the definition.

A sample has a history x_l (l < L) of width D and a candidate doc of width Dq; H = head_num heads of width d = att_embedding_size, E = H d;
weights W_query (Dq, E), W_key (D, E), W_value (D, E), head h owning columns h d .. (h + 1) d - 1.  Over the key positions K (l < lengths and
mask != 0):

    Q = doc W_query,   K_l = x_l W_key,   V_l = x_l W_value                          per head
    a_h = softmax over l in K of <Q_h, K_lh>  (times 1 / sqrt(d) with scaling=True)
    out = concat_h sum_l a_hl V_lh                                                  (B, E)

No position is projected: <Q_h, x_l W_key,h> = <W_key,h Q_h, x_l>, so the key projection is folded into a (B, H, D) query k~ = W_key,h Q_h;
the kernel of attention_by_softmax (csrc/attention_softmax.hip) streams the (B, L, D) history once per direction against k~ and pools it to
a (B, H, D) context, and sum_l a_hl x_l W_value,h = context_h W_value,h because the weights of a sample with a key sum to 1.  The three small
projections are torch ops under autograd.  A sample without a key gives a zero row.  No output projection, dropout or positional bias.

Symbols: B batch size, L history length, D embedding dim, Dq candidate dim, H head_num, d att_embedding_size, E = H d.
"""
import math

import torch

from ._keras import Layer, get_initializer


class TargetAttentionLayer(Layer):
    """Multi-head softmax attention pooling of a padded (B, L, D) history with the candidate item as the query."""

    def __init__(self, head_num=2, att_embedding_size=8, scaling=True, kernel_initializer='glorot_uniform', kernel_regularizer=None,
                 kernel_constraint=None, **kwargs):
        """
        Args:
            head_num: H, the number of heads (the kernels cover H <= 8).
            att_embedding_size: d, the width of a head; the output has H d columns.
            scaling: multiply the scores by 1 / sqrt(d).
            kernel_initializer: a name of _keras.get_initializer or a callable, drawn per matrix.
            kernel_regularizer, kernel_constraint: kept with every matrix, as add_weight does.
        """
        super().__init__(**kwargs)
        if int(head_num) < 1:
            raise ValueError('head_num must be >= 1, got %r' % (head_num,))
        if int(att_embedding_size) < 1:
            raise ValueError('att_embedding_size must be >= 1, got %r' % (att_embedding_size,))
        self.head_num = int(head_num)
        self.att_embedding_size = int(att_embedding_size)
        self.scaling = bool(scaling)
        self.kernel_initializer = kernel_initializer
        self.kernel_regularizer = kernel_regularizer
        self.kernel_constraint = kernel_constraint

    def build(self, input_shape):
        """input_shape: ((B, L, D), (B, Dq)).  Creates W_query (Dq, E), W_key (D, E) and W_value (D, E)."""
        D, Dq = int(input_shape[0][-1]), int(input_shape[1][-1])
        E = self.head_num * self.att_embedding_size
        kw = dict(initializer=get_initializer(self.kernel_initializer), regularizer=self.kernel_regularizer, constraint=self.kernel_constraint)
        self.W_query = self.add_weight('W_query', (Dq, E), **kw)
        self.W_key = self.add_weight('W_key', (D, E), **kw)
        self.W_value = self.add_weight('W_value', (D, E), **kw)
        self.built = True

    def forward(self, user_emb, doc_emb, lengths=None, mask=None):
        for t, what in ((user_emb, 'user_emb'), (doc_emb, 'doc_emb')):
            if not isinstance(t, torch.Tensor):
                raise TypeError('%s must be a torch.Tensor, got %s' % (what, type(t)))
        if user_emb.dim() != 3 or doc_emb.dim() != 2 or user_emb.shape[0] != doc_emb.shape[0]:
            raise ValueError('user_emb must be (B, L, D) and doc_emb (B, Dq); got %s and %s' % (tuple(user_emb.shape), tuple(doc_emb.shape)))
        if not self.built:
            self._build_device = user_emb.device
            self.build((tuple(user_emb.shape), tuple(doc_emb.shape)))
        return self.call(user_emb, doc_emb, lengths=lengths, mask=mask)

    def call(self, user_emb, doc_emb, lengths=None, mask=None):
        """user_emb (B, L, D), doc_emb (B, Dq) float32 GPU tensors; lengths (B,) integers and / or mask (B, L), as attention_by_softmax
        takes them -> (B, E)."""
        from ..rec_block.attention import attention_by_softmax     # here: rec_block.attention itself imports this package's _keras
        B, L, D = user_emb.shape
        H, d = self.head_num, self.att_embedding_size
        E = H * d
        for name, shape in (('W_query', (doc_emb.shape[1], E)), ('W_key', (D, E)), ('W_value', (D, E))):
            if tuple(getattr(self, name).shape) != shape:
                raise ValueError('%s has shape %s; a history of width %d and a candidate of width %d with %d heads of width %d need %s'
                                 % (name, tuple(getattr(self, name).shape), D, doc_emb.shape[1], H, d, shape))
        q = (doc_emb @ self.W_query).reshape(B, H, d)
        folded = torch.einsum('dhe,bhe->bhd', self.W_key.reshape(D, H, d), q)               # k~[b, h] = W_key,h Q[b, h]
        context = attention_by_softmax(user_emb, folded, lengths=lengths, mask=mask, scale=1.0 / math.sqrt(d) if self.scaling else 1.0)
        return torch.einsum('bhd,dhe->bhe', context, self.W_value.reshape(D, H, d)).reshape(B, E)
