"""Device arrays between guard bytes, for the GPU tests whose outputs must not be written past their ends."""
import numpy as np
import torch

DEV = "cuda:0"
G, FILL = 64, 0xEE  # guard bytes on both sides of every array, and what they (and a fresh array) hold


class Guarded:
    """nbytes on the device between two guards of `guard` bytes of FILL; `t` is the part handed to the call, as
    `dtype`, holding `init` (any array, by its bytes) or else `fill`."""

    def __init__(self, nbytes, init=None, fill=FILL, dtype=torch.uint8, guard=G):
        self.big = torch.full((nbytes + 2 * guard,), FILL, dtype=torch.uint8, device=DEV)
        self.n, self.g = nbytes, guard
        self.t = self.big[guard:guard + nbytes].view(dtype)
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).reshape(-1)))
        elif fill != FILL:
            self.t.fill_(fill)

    def host(self, dtype=np.uint8):
        b = self.big.cpu().numpy()
        assert (b[:self.g] == FILL).all() and (b[self.g + self.n:] == FILL).all(), "written outside the array"
        return b[self.g:self.g + self.n].copy().view(dtype)
