"""Guard bands, poisons and const checks for buffers handed to the C ABI (plain functions, like tests/routing_util.py).

A guarded buffer is a view of ``n_elems`` elements inside a larger backing tensor ``[front guard | payload | back guard]``.  Both
guards hold one fixed 32-bit pattern, a NaN with a recognisable payload, and are compared as integer bits (never as floats: NaN != NaN).
A store of a kernel before the start or past the end of the buffer it was given lands in a guard and is reported with its offsets.

What this cannot see: out-of-range READS (a guard is not changed by them), and stores that jump over a whole guard (4 096 elements or
more away from the buffer).  A green run says "no store next to the buffer, nothing read from poisoned memory that reached an output",
not "memory safe".
"""
import torch

GUARD_ELEMS = 4096
GUARD_WORD = 0x7FC5A17E            # as fp32: a quiet NaN with payload 0x05A17E
NAN64_WORD = 0x7FF8A17E7FC5A17E    # the NaN poison of an fp64 payload (two guard words side by side would be a finite double)
POISON_NAN = "nan"
POISON_FINITE = "finite"
_FINITE = {torch.float32: 3e38, torch.float64: 1e300}


class Guarded:
    """view: the payload (what the kernel is given); backing: the whole allocation as bytes."""

    def __init__(self, name, view, backing, front_bytes, payload_bytes):
        self.name, self.view, self.backing = name, view, backing
        self.front_bytes, self.payload_bytes = front_bytes, payload_bytes

    def guard_words(self, side):
        raw = self.backing
        if side == "front":
            return raw[:self.front_bytes].view(torch.int32)
        start = self.front_bytes + self.payload_bytes
        start_al = (start + 3) // 4 * 4             # byte payloads: the back guard's words start at the next 4-byte boundary ...
        return raw[start_al:].view(torch.int32), raw[start:start_al]      # ... and the bytes in between are checked one by one


def poison_value(dtype, fill):
    """The scalar a poisoned payload holds (None for the NaN bit pattern, which is written as words)."""
    if fill == POISON_FINITE:
        if dtype in _FINITE:
            return _FINITE[dtype]
        return 0x5A if dtype == torch.uint8 else 0x5A5A5A5A
    return None


def guarded(n_elems, dtype, device, fill, shift_elems=0, name="buffer"):
    """A Guarded whose .view has n_elems elements of dtype.  fill: a tensor with n_elems elements (real data), POISON_NAN or POISON_FINITE,
    or a number.  shift_elems = 0: the payload is 16-byte aligned; 1: it starts one element later (data_ptr() % 16 == element size for
    4- and 8-byte types; 4 bytes later for byte buffers)."""
    esize = torch.empty((), dtype=dtype).element_size()
    n_elems = int(n_elems)
    front = GUARD_ELEMS * 4 + 16                      # room to place the payload on a 16-byte boundary, then to shift it
    payload = n_elems * esize
    total = front + 16 + payload + 16 + GUARD_ELEMS * 4
    total = (total + 3) // 4 * 4
    backing = torch.empty(total, dtype=torch.uint8, device=device)
    backing.view(torch.int32).fill_(GUARD_WORD)
    base = backing.data_ptr()
    assert base % 4 == 0
    off = front + (-(base + front)) % 16 + int(shift_elems) * max(esize, 4)      # byte buffers move by 4 bytes: every address stays 4-byte aligned
    assert off % esize == 0 or (base + off) % esize == 0
    view = backing[off:off + payload].view(dtype) if n_elems else backing[off:off].view(dtype)
    if shift_elems == 0:
        assert view.data_ptr() % 16 == 0 or n_elems == 0
    elif esize in (4, 8) and n_elems:
        assert view.data_ptr() % 16 == (int(shift_elems) * esize) % 16
    if isinstance(fill, torch.Tensor):
        assert fill.numel() == n_elems and fill.dtype == dtype, (name, fill.numel(), n_elems, fill.dtype, dtype)
        view.copy_(fill.reshape(-1).to(device))
    elif fill == POISON_NAN:
        if esize == 8:
            view.view(torch.int64).fill_(NAN64_WORD)
        elif esize == 4:
            view.view(torch.int32).fill_(GUARD_WORD)
        else:
            view.fill_(0x7E)
    elif fill == POISON_FINITE:
        view.fill_(poison_value(dtype, fill))
    else:
        view.fill_(fill)
    return Guarded(name, view, backing, off, payload)


def _damage(words, pattern):
    bad = (words != pattern).nonzero().flatten()
    if bad.numel() == 0:
        return None
    return int(bad[0]), int(bad[-1]), int(bad.numel())


def guard_damage(g):
    """[] when both guards of g are intact, else a list of (side, first, last, count): offsets in 32-bit words, counted from the buffer's
    edge outwards for the front guard (1 = the word just before the payload) and from its end for the back guard (0 = the word just
    past it)."""
    out = []
    front = g.guard_words("front")
    d = _damage(front, GUARD_WORD)
    if d:
        n = front.numel()
        out.append(("front", n - d[1], n - d[0], d[2]))
    back, gap = g.guard_words("back")
    pat = torch.tensor([GUARD_WORD], dtype=torch.int32).view(torch.uint8)
    gap_start = g.front_bytes + g.payload_bytes
    gap_bad = [i for i in range(gap.numel()) if int(gap[i]) != int(pat[(gap_start + i) % 4])]
    d = _damage(back, GUARD_WORD)
    if d or gap_bad:
        first = 0 if gap_bad else d[0] + (1 if gap.numel() else 0)
        last = d[1] + (1 if gap.numel() else 0) if d else 0
        out.append(("back", first, last, (d[2] if d else 0) + (1 if gap_bad else 0)))
    return out


def assert_guards_intact(buffers, sync=None):
    """buffers: iterable of Guarded.  Call after torch.cuda.synchronize() (or pass it as ``sync``)."""
    if sync is not None:
        sync()
    problems = []
    for g in buffers:
        for side, first, last, count in guard_damage(g):
            problems.append("%s: %s guard damaged, %d word(s), first at word offset %d, last at %d" % (g.name, side, count, first, last))
    assert not problems, "; ".join(problems)


def bits(t):
    """The bits of a tensor as an integer tensor of the same length on the CPU (a copy)."""
    t = t.detach().contiguous().reshape(-1)
    kind = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.view(kind).cpu().clone()


def assert_unchanged(input_view, saved_bits, name="input"):
    """A ``const`` argument after the call: bit for bit what bits() returned before it."""
    now = bits(input_view)
    bad = (now != saved_bits).nonzero().flatten()
    assert bad.numel() == 0, "%s: input modified, %d element(s), first at %d, last at %d" % (name, bad.numel(), int(bad[0]), int(bad[-1]))


def poison_left(view, fill):
    """Indices of the elements of an output that still hold the poison (never written)."""
    if fill == POISON_NAN:
        if view.element_size() == 8:
            return (view.contiguous().reshape(-1).view(torch.int64) == NAN64_WORD).nonzero().flatten()
        if view.element_size() == 4:
            return (view.contiguous().reshape(-1).view(torch.int32) == GUARD_WORD).nonzero().flatten()
        return (view.reshape(-1) == 0x7E).nonzero().flatten()
    return (view.reshape(-1) == poison_value(view.dtype, fill)).nonzero().flatten()
