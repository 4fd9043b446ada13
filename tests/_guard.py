"""Guard-banded device buffers of the C-ABI route tests: sentinel words around every buffer, NaN inside it before a call."""
import numpy as np

SENT = 0x7FC0DEAD                  # sentinel word (a NaN no kernel computes)
TAIL = 1024                        # sentinel words past every buffer


class Buf:
    """`lead` sentinel words, n fp32 words (NaN, or `data`), TAIL sentinel words; ptr addresses the first of the n words.  The allocation is
    256-byte aligned, so ptr is `lead` floats past a 16-byte boundary."""

    def __init__(self, dev, n, data=None, lead=0):
        import torch
        self.n, self.lead = int(n), int(lead)
        self.buf = torch.full((self.lead + self.n + TAIL,), float('nan'), dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self._sent = np.int32(np.uint32(SENT).view(np.int32))
        self.buf.view(torch.int32)[:self.lead].fill_(self._sent)
        self.buf.view(torch.int32)[self.lead + self.n:].fill_(self._sent)
        self.body = self.buf[self.lead:self.lead + self.n]
        if data is not None:
            self.body.copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32).reshape(-1)).to(dev))
        self.ptr = self.buf.data_ptr() + 4 * self.lead

    def nan(self):
        self.body.fill_(float('nan'))

    def damaged(self):
        import torch
        w = self.buf.view(torch.int32)
        return int((w[:self.lead] != self._sent).sum()) + int((w[self.lead + self.n:] != self._sent).sum())

    def get(self, shape):
        return self.body.cpu().numpy().reshape(shape)

    def untouched(self):
        """every word of the body is still the NaN it was filled with"""
        import torch
        return bool(torch.isnan(self.body).all())
