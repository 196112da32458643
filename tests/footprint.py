"""Shared helpers of the memory-footprint tests (test_memory_footprint_cpu.py, test_memory_footprint_gpu.py, footprint_child.py).
TEST INFRASTRUCTURE: which cells of the input a launch may depend on, inputs poisoned with NaN everywhere else, comparisons that
see NaN payloads (through an integer view), and host arrays placed flush against inaccessible pages."""
import ctypes
import mmap

import numpy as np

import oracle

# quiet NaNs with a payload: "the ring is still the NaN it was" is a statement about bits, not about isnan()
NAN_BITS = {np.dtype(np.float32): 0x7FC0DEAD, np.dtype(np.float64): 0x7FF8DEAD0000BEEF}
_UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def bits(a):
    """The array's bit patterns (np.array_equal on floats treats NaN as unequal to itself)."""
    a = np.ascontiguousarray(a)
    return a.view(_UINT[a.dtype])


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


def nan_value(dtype):
    dt = np.dtype(dtype)
    return np.array([NAN_BITS[dt]], dtype=_UINT[dt]).view(dt)[0]


def nan_filled(shape, dtype):
    a = np.empty(shape, dtype=dtype)
    bits(a)[...] = NAN_BITS[np.dtype(dtype)]
    return a


def is_poison(a):
    """True where `a` holds exactly the poison NaN."""
    return bits(a) == NAN_BITS[np.ascontiguousarray(a).dtype]


def interior_slices(shape, h):
    return tuple(slice(h, n - h) for n in shape)


def ring_mask(shape, h):
    ring = np.ones(shape, bool)
    ring[interior_slices(shape, h)] = False
    return ring


def read_mask(spec):
    """Boolean array of spec.shape: true where some interior output point has a tap (the union over spec.points of the interior box
    shifted by the tap).  `spec` is the fused oracle.Spec, so this is the footprint of ONE launch; everything else in the input --
    ring corners and edges for stars and crosses, more for one-sided shapes -- is memory a launch has no business depending on."""
    shape = tuple(spec.shape)
    nd = len(shape)
    h = spec.halo
    m = np.zeros(shape, bool)
    for off, _ in spec.points:
        off = tuple(off)[3 - nd:]
        assert all(0 <= h + o and n - h + o <= n for o, n in zip(off, shape)), "a tap reaches beyond the ring"
        m[tuple(slice(h + o, n - h + o) for o, n in zip(off, shape))] = True
    return m


def poison(A0, spec):
    """Copy of A0 with NaN wherever read_mask is false.  Asserts the precondition "the reference stays clean": one oracle sweep of
    the poisoned input into an all-NaN output gives a NaN-free interior (and leaves the output's ring alone)."""
    P = np.ascontiguousarray(A0).copy()
    P[~read_mask(spec)] = nan_value(P.dtype)
    B = nan_filled(P.shape, P.dtype)
    oracle.sweep(spec, P, B, contract=1)
    assert not np.isnan(spec.interior(B)).any(), "the oracle's own sweep of the poisoned input is not NaN-free"
    assert is_poison(B)[ring_mask(B.shape, spec.halo)].all(), "the oracle's sweep wrote the ring"
    return P


def poison_periodic(A0, spec):
    """--boundary periodic: every interior cell is read (by the stencil or as somebody's image) and the whole ring is WRITTEN by the
    wrap from the interior before anything reads it, so the ring is what a launch must not depend on: NaN in all of it."""
    P = np.ascontiguousarray(A0).copy()
    P[ring_mask(P.shape, spec.halo)] = nan_value(P.dtype)
    return P


# ---- host arrays flush against PROT_NONE pages (CPU only) ----------------------------------------------------------------------------
PAGE = mmap.PAGESIZE
PROT_NONE = 0          # <sys/mman.h>; the mmap module has no name for it
_libc = None


def _c():
    global _libc
    if _libc is None:
        _libc = ctypes.CDLL(None, use_errno=True)
        _libc.mmap.restype = ctypes.c_void_p
        _libc.mmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long]
        _libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _libc.munmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    return _libc


class Guarded:
    """An array of `shape` in an anonymous mapping with an inaccessible page before and after.  placement "end": the array's last
    byte is the last byte before the trailing page; "start": its first byte is the first byte behind the leading page.  Any access
    past that edge is a SIGSEGV, so this is used in child processes only."""

    def __init__(self, shape, dtype, placement):
        assert placement in ("end", "start")
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dt.itemsize
        body = -(-nbytes // PAGE) * PAGE
        self.length = body + 2 * PAGE
        base = _c().mmap(None, self.length, mmap.PROT_READ | mmap.PROT_WRITE, mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, -1, 0)
        assert base not in (None, ctypes.c_void_p(-1).value), "mmap failed: errno %d" % ctypes.get_errno()
        self.base = base
        for page in (base, base + PAGE + body):
            assert _c().mprotect(page, PAGE, PROT_NONE) == 0, "mprotect failed: errno %d" % ctypes.get_errno()
        self.addr = base + PAGE + (body - nbytes if placement == "end" else 0)
        self._buf = (ctypes.c_char * nbytes).from_address(self.addr)
        self.array = np.frombuffer(self._buf, dtype=dt).reshape(shape)
        assert self.array.ctypes.data == self.addr and self.array.flags.writeable

    def close(self):
        if self.base is not None:
            self.array = self._buf = None
            _c().munmap(self.base, self.length)
            self.base = None


# ---- device-side twins (torch tensors; the full-size GPU cases never bring a whole array to the host) -------------------------------
def read_mask_torch(torch, spec, device):
    """read_mask() as a torch.bool tensor on `device`."""
    shape = tuple(spec.shape)
    nd = len(shape)
    h = spec.halo
    m = torch.zeros(shape, dtype=torch.bool, device=device)
    for off, _ in spec.points:
        off = tuple(off)[3 - nd:]
        m[tuple(slice(h + o, n - h + o) for o, n in zip(off, shape))] = True
    return m


def int_view(torch, t):
    """A float tensor's bit patterns (torch.equal on floats treats NaN as unequal to itself)."""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)
