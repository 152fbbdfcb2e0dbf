"""What the kernel-by-kernel GPU tests share (tests/test_gpu_param_prologue.py, tests/test_gpu_param_backward.py): outputs kept
between guard words filled with a NaN bit pattern no kernel produces, and the value families of the logits."""
import torch

NAN_BITS = 0x7FC0DEAD
GUARD = 64  # words: 256 bytes, so a guarded output keeps the 16-byte alignment of the allocation
NEG_INF = float("-inf")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _Guarded:
    """n fp32 words of output between two guard blocks (`lead` extra words in front shift it off 16-byte alignment)."""

    def __init__(self, n, dev, lead=0):
        self.n, self.lo = int(n), GUARD + lead
        self.bits = torch.full((self.lo + self.n + GUARD,), NAN_BITS, dtype=torch.int32, device=dev)
        self.out = self.bits[self.lo:self.lo + self.n].view(torch.float32)

    def raw(self):
        """The owned words as int32 on the host, guards checked."""
        b = self.bits.cpu()
        assert bool((b[:self.lo] == NAN_BITS).all()), "words BEFORE the output were overwritten"
        assert bool((b[self.lo + self.n:] == NAN_BITS).all()), "words AFTER the output were overwritten"
        return b[self.lo:self.lo + self.n]

    def read(self, owned=None):
        """The output on the host; `owned`: bool mask of the words the kernel must write (default all) -- the others must
        still hold the fill pattern."""
        b = self.raw()
        written = b != NAN_BITS
        if owned is None:
            assert bool(written.all()), f"{int((~written).sum())} of {self.n} owned words were never written"
        else:
            owned = owned.reshape(-1)
            assert bool(written[owned].all()), f"{int((~written[owned]).sum())} owned words were never written"
            assert not bool(written[~owned].any()), f"{int(written[~owned].sum())} words the kernel does not own were written"
        return b.view(torch.float32)


def _logits(shape, fam, g):
    """fp32 logits of a value family; the softmax axis is the last one.  'neginf' keeps one column finite in every row."""
    x = torch.randn(shape, generator=g)
    if fam == "shift+":
        x = x + 1e4
    elif fam == "shift-":
        x = x - 1e4
    elif fam == "spread":
        x = torch.rand(shape, generator=g) * 200 - 100
    elif fam == "const":
        x = torch.full(shape, 0.75)
    elif fam == "neginf" and shape[-1] > 1:
        m = torch.rand(shape, generator=g) < 0.3
        m[..., int(torch.randint(shape[-1], (1,), generator=g))] = False
        x[m] = NEG_INF
    return x.contiguous()
