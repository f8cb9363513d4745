"""A test field of the kernel ABI at ANY accepted layout — TEST INFRASTRUCTURE ONLY (the product and bench.py use
gpusolve.devfield.DevField, which knows gs_field_layout's layout alone).

include/gpusolve_hip.h accepts every pitch ldy >= nx+2, ldz >= ldy*(ny+2) and any 8-byte-aligned field pointer.
LayoutField(nx, ny, nz, ldy, ldz, phase) builds one such field inside a torch float64 buffer:

    [ guard margin | plane -1 | planes 0 .. nz+1 (the padded box lives here) | plane nz+2 | guard margin ]

with planes of ldz elements, rows of ldy, a margin of 2*ldz + 64 elements on each side, and the byte address of padded
element (x=1, y=0, z=0) equal to `phase` modulo 128. Everything that is not the padded box — pitch padding, the gap
between planes, the second ghost planes, the margins — can be poisoned with a NaN of a recognisable payload, inputs
and outputs alike, so a test sees (a) every word a launcher writes, (b) every word of an input it changes and (c) any
word outside the box whose value reaches a result. device="cpu" gives the same object on host memory (the helper's
own tests, tests/test_layout_field_cpu.py)."""
from collections import namedtuple

import numpy as np
import torch

POISON_IN = 0x7FF8_C0DE_0000_0A11   # a quiet NaN: inputs outside their padded box
POISON_OUT = 0x7FF8_DEAD_0000_0B22  # a quiet NaN: outputs before the call

Layout = namedtuple("Layout", "id ldy ldz phase_in phase_out aligned")
LAYOUT_IDS = ("default", "tight_even", "loose", "tight_odd", "mixed")
ALIGNED_IDS = ("default", "tight_even", "loose")


def default_pitches(nx, ny, nz):
    """gs_field_layout's pitches, restated (tests/test_layout_field_cpu.py holds it to the library's)."""
    ldy = (nx + 2 + 15) // 16 * 16
    return ldy, ldy * (ny + 2)


def layouts(nx, ny, nz):
    """The named layouts for a level of interior (nx, ny, nz): id -> Layout. phase_in is the phase of x=1 of the
    call's input fields, phase_out that of its outputs and of f (they differ in `mixed` only)."""
    D, Dz = default_pitches(nx, ny, nz)
    even = nx + 2 + (nx + 2) % 2
    odd = nx + 2 + (nx + 1) % 2
    odd_z = odd * (ny + 2)
    odd_z += (odd_z + 1) % 2
    out = [
        Layout("default", D, Dz, 0, 0, True),
        Layout("tight_even", even, even * (ny + 2), 16, 16, True),
        Layout("loose", D + 6, (D + 6) * (ny + 2) + 10, 64, 64, True),
        Layout("tight_odd", odd, odd_z, 8, 8, False),
        Layout("mixed", D, Dz, 0, 8, False),
    ]
    return {l.id: l for l in out}


class LayoutField:
    def __init__(self, nx, ny, nz, ldy, ldz, phase, device="cuda"):
        assert ldy >= nx + 2 and ldz >= ldy * (ny + 2), "not a layout the ABI accepts"
        assert 0 <= phase < 128 and phase % 8 == 0
        self.nx, self.ny, self.nz, self.ldy, self.ldz, self.phase = nx, ny, nz, ldy, ldz, phase
        self.margin = 2 * ldz + 64
        self.planes = (nz + 4) * ldz  # planes -1 .. nz+2
        self.buf = torch.zeros(self.margin + 16 + self.planes + self.margin, dtype=torch.float64, device=device)
        base = self.buf.data_ptr()
        assert base % 8 == 0
        o = self.margin + ldz  # the first candidate for padded element (0, 0, 0); 16 elements are one 128-byte period
        o += ((phase - (base + 8 * (o + 1))) % 128) // 8
        self.origin = o
        self.ptr = base + 8 * o
        assert (self.ptr + 8) % 128 == phase
        self.i64 = self.buf.view(torch.int64)
        self._snap = self._poison = None

    # ---- views ------------------------------------------------------------------------------------------------
    def _box(self, t):
        """[z][y][x] view of the padded box of a whole-buffer tensor."""
        return torch.as_strided(t, (self.nz + 2, self.ny + 2, self.nx + 2), (self.ldz, self.ldy, 1), self.origin)

    def _ext(self, t):
        """The same with the second ghost planes: z = -1 .. nz+2."""
        return torch.as_strided(t, (self.nz + 4, self.ny + 2, self.nx + 2), (self.ldz, self.ldy, 1),
                                self.origin - self.ldz)

    def level(self, h, z0=0):
        from gpusolve import gs_level
        return gs_level(self.nx, self.ny, self.nz, self.ldy, self.ldz, z0, h)

    def _sync(self):
        if self.buf.is_cuda:
            torch.cuda.synchronize()

    def to_xyz(self):
        self._sync()
        return np.ascontiguousarray(self._box(self.buf).cpu().numpy().transpose(2, 1, 0))

    def to_xyz_ext(self):
        self._sync()
        return np.ascontiguousarray(self._ext(self.buf).cpu().numpy().transpose(2, 1, 0))

    def from_xyz(self, arr):
        a = np.asarray(arr, dtype=np.float64)
        assert a.shape == (self.nx + 2, self.ny + 2, self.nz + 2), a.shape
        self._box(self.buf)[...] = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 1, 0))).to(self.buf.device)
        return self

    def from_xyz_ext(self, arr):
        """Planes z = -1 .. nz+2 from an array shaped (nx+2, ny+2, nz+4)."""
        a = np.asarray(arr, dtype=np.float64)
        assert a.shape == (self.nx + 2, self.ny + 2, self.nz + 4), a.shape
        self._ext(self.buf)[...] = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 1, 0))).to(self.buf.device)
        return self

    # ---- masks over the whole buffer --------------------------------------------------------------------------
    def _mask(self):
        return torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)

    def box_mask(self):
        m = self._mask()
        self._box(m)[...] = True
        return m

    def interior_mask(self):
        m = self._mask()
        self._box(m)[1:-1, 1:-1, 1:-1] = True
        return m

    def ext_box_mask(self):
        """The padded box plus the box-shaped part of planes -1 and nz+2."""
        m = self._mask()
        self._ext(m)[...] = True
        return m

    def planes_mask(self):
        """Planes -1 .. nz+2 at full pitch (what gs_newton_bfac writes)."""
        m = self._mask()
        m[self.origin - self.ldz: self.origin - self.ldz + self.planes] = True
        return m

    # ---- poison -------------------------------------------------------------------------------------------------
    def poison_outside_box(self, word=POISON_IN, keep=None):
        """Every word outside the padded box (outside `keep`, a whole-buffer mask, when given) becomes `word`."""
        self.i64[~(self.box_mask() if keep is None else keep)] = word
        return self

    def poison_all(self, word=POISON_OUT):
        self.i64.fill_(word)
        self._poison = word
        return self

    # ---- checks -------------------------------------------------------------------------------------------------
    def snapshot(self):
        self._sync()
        self._snap = self.i64.clone()
        return self

    def assert_unchanged(self, mask=None, what=""):
        """Every word (of `mask`) holds what it held at snapshot(), bit for bit."""
        self._sync()
        diff = self.i64 != self._snap
        if mask is not None:
            diff &= mask
        if bool(diff.any()):
            i = int(torch.nonzero(diff)[0])
            raise AssertionError(f"{what}: word {self.describe(i)} changed "
                                 f"({int(self._snap[i]):#018x} -> {int(self.i64[i]):#018x}); {int(diff.sum())} in all")

    def assert_written_exactly(self, mask, what=""):
        """After poison_all(): every word of `mask` was written, and no other word."""
        self._sync()
        written = self.i64 != self._poison
        stray = written & ~mask
        if bool(stray.any()):
            i = int(torch.nonzero(stray)[0])
            raise AssertionError(f"{what}: word {self.describe(i)} outside the documented set was written "
                                 f"({int(stray.sum())} in all)")
        missed = mask & ~written
        if bool(missed.any()):
            i = int(torch.nonzero(missed)[0])
            raise AssertionError(f"{what}: word {self.describe(i)} of the documented set was not written "
                                 f"({int(missed.sum())} in all)")

    def describe(self, i):
        """Buffer index -> 'buf[i] = (x, y, z) + where it lies'."""
        r = i - self.origin
        z, r2 = r // self.ldz, r % self.ldz
        y, x = r2 // self.ldy, r2 % self.ldy
        if not -1 <= z <= self.nz + 2:
            return f"buf[{i}] (guard margin, {r} elements from the origin)"
        kind = ("box" if 0 <= z <= self.nz + 1 and y <= self.ny + 1 and x <= self.nx + 1 else
                "ghost plane" if y <= self.ny + 1 and x <= self.nx + 1 else
                "pitch padding" if y <= self.ny + 1 else "plane gap")
        return f"buf[{i}] = (x={x}, y={y}, z={z}) [{kind}]"
