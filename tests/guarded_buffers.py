"""What the kernel-by-kernel GPU tests share (tests/test_gpu_param_prologue.py, tests/test_gpu_param_backward.py,
tests/test_gpu_layer_backward.py): outputs kept between guard words filled with a NaN bit pattern no kernel produces -- one output,
or an arena of several blocks in one allocation -- and the value families of the logits."""
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


class _GuardedArena:
    """Several fp32 blocks (`sizes`, in words) in ONE allocation with guard words in front of, between and behind them: the
    gradient arena of a layer backward, whose kernels receive the base pointer and word offsets (`off`, every one a multiple of
    4 words).  `lead` extra words in front shift the base off 16-byte alignment.  Words of blocks nobody filled keep the NaN
    pattern like the guards."""

    def __init__(self, sizes, dev, lead=0):
        self.sizes, self.off = [int(n) for n in sizes], []
        at = GUARD
        for n in self.sizes:
            self.off.append(at)
            at = (at + n + 3) // 4 * 4 + GUARD
        self.words, self.lead = at, lead
        self.bits = torch.full((lead + at,), NAN_BITS, dtype=torch.int32, device=dev)
        self.base = self.bits[lead:].view(torch.float32)
        self.prior = None

    def ptr(self):
        return self.base.data_ptr()

    def fill(self, values):
        """values: one flat fp32 host tensor per block -> the blocks (the prior a kernel adds to, or an input arena)."""
        host = torch.full((self.words,), NAN_BITS, dtype=torch.int32)
        for o, n, v in zip(self.off, self.sizes, values):
            host[o:o + n] = v.reshape(-1).view(torch.int32)
        self.prior = host
        self.bits[self.lead:].copy_(host)
        return host.view(torch.float32)

    def block_mask(self, blocks):
        m = torch.zeros(self.words, dtype=torch.bool)
        for i in blocks:
            m[self.off[i]:self.off[i] + self.sizes[i]] = True
        return m

    def read(self, targets):
        """The arena on the host (fp32, from the base).  `targets`: indices of the blocks the kernel must write.  Not filled:
        every word of every target block was written and every other word still holds the pattern.  Filled with a prior: every
        word outside the target blocks holds exactly what it held."""
        b = self.bits.cpu()
        assert bool((b[:self.lead] == NAN_BITS).all()), "words BEFORE the arena were overwritten"
        b = b[self.lead:]
        own = self.block_mask(targets)
        if self.prior is None:
            written = b != NAN_BITS
            assert bool(written[own].all()), f"{int((~written[own]).sum())} words of the targeted blocks were never written"
            assert not bool(written[~own].any()), f"{int(written[~own].sum())} words outside the targeted blocks were written"
        else:
            assert torch.equal(b[~own], self.prior[~own]), "a word outside the targeted blocks (a guard or another block) changed"
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
