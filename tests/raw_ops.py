"""Thin functional wrapper over the C ABI used by the tests.

`RawOps("hip")` drives libm355seg.so with CUDA tensors; `RawOps("oracle")` drives
oracle/libm355_oracle.so (same signatures, m355o_ prefix) with CPU tensors.  The
parity tests run the same call on both and compare.
"""
import ctypes as C
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from segmentation_pipeline_amd import _lib  # noqa: E402
from segmentation_pipeline_amd._lib import ConvDesc, NormDesc  # noqa: E402

ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_LIB = os.environ.get("M355_ORACLE_LIB") or os.path.join(ORACLE_DIR, "libm355_oracle.so")  # override: the ASan build (oracle/Makefile)


def build_oracle():
    src = os.path.join(ORACLE_DIR, "m355_oracle.c")
    if (not os.path.exists(ORACLE_LIB)) or os.path.getmtime(ORACLE_LIB) < os.path.getmtime(src):
        subprocess.run(["make", "-C", ORACLE_DIR], check=True, capture_output=True)
    return ORACLE_LIB


class Slot:
    """A tensor embedded as a channel slice of a larger, canary-filled flat buffer -- what `ops.OutSlot` /
    `ops._dense_channels` (fp32) and `ops.Act16.slot` (c8) hand to the library, plus guards a test can inspect.

    `shape` is the logical tensor: fp32 [N, C, D, H, W], or c8 [N, CB, S, 8] (then the "channels" below are channel
    blocks).  Flat layout, in elements, `unit` = elements of one channel:

        guard | lead | n = 0: c_pre * unit | C * unit (the slot) | c_post * unit | extra | n = 1: ... | guard

    so the batch stride is (c_pre + C + c_post) * unit + extra, and the pointer handed to the library sits
    (lead + c_pre * unit) elements behind a 64-byte aligned address.  `guard` is at least one full channel and at least
    64 elements, a multiple of 16 elements.  Everything that is not the slot holds one quiet-NaN bit pattern of the element
    type (compared through an integer view: bit-exact); so does the inside of an output slot (`data` is None).  An
    input slot holds `data`.  A kernel that reads outside its slot and uses the value turns its result NaN."""

    CANARY = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.bfloat16: (torch.int16, 0x7FC5),
              torch.float16: (torch.int16, 0x7E55)}

    def __init__(self, device, shape, c_pre=1, c_post=1, lead=0, extra=0, dtype=torch.float32, data=None):
        if data is not None:
            shape, dtype = tuple(data.shape), data.dtype
        self.shape, self.dtype, self.device = torch.Size(shape), dtype, device
        N, Cc = shape[0], shape[1]
        unit = 1
        for v in shape[2:]:
            unit *= v
        assert N >= 1 and Cc >= 1 and unit >= 1 and min(c_pre, c_post, lead, extra) >= 0
        itype, self.canary = self.CANARY[dtype]
        self.unit = unit
        self.bs = (c_pre + Cc + c_post) * unit + extra
        self.bs_arg = self.bs    # what the wrappers pass as batch stride (the harness self-test passes a wrong one on purpose)
        guard = -(-max(unit, 64) // 16) * 16
        self.off = guard + lead + c_pre * unit
        self.ibuf = torch.full((guard + lead + N * self.bs + guard,), self.canary, dtype=itype, device=device)
        assert self.ibuf.data_ptr() % 64 == 0, "allocator alignment the layout classes are built on"
        self.ptr = self.ibuf.data_ptr() + self.off * self.ibuf.element_size()
        self.is_input = data is not None
        if data is not None:
            self.view().copy_(data.to(device))
        self.before = self.ibuf.clone()

    def _strided(self, flat):
        st, acc = [], 1
        for v in reversed(self.shape[2:]):
            st.append(acc)
            acc *= v
        return torch.as_strided(flat, self.shape, (self.bs, self.unit) + tuple(reversed(st)), self.off)

    def view(self):
        """the slot as a strided view of the buffer, in the element type"""
        return self._strided(self.ibuf.view(self.dtype))

    def numel(self):
        return self.shape.numel()

    def misalign(self, to=16):
        """bytes the slot pointer is off a `to`-byte boundary"""
        return self.ptr % to

    def result(self):
        return self.view().clone(memory_format=torch.contiguous_format)

    def assert_guards_intact(self, what=""):
        g = self.ibuf.clone()
        self._strided(g).fill_(self.canary)
        bad = (g != self.canary).nonzero().flatten()
        assert bad.numel() == 0, (f"{what}: {bad.numel()} elements outside the slot were overwritten; first at flat offset "
                                  f"{int(bad[0])} (slot starts at {self.off}, batch stride {self.bs}, channel {self.unit})")

    def assert_fully_written(self, what=""):
        left = (self._strided(self.ibuf) == self.canary)
        assert not bool(left.any()), f"{what}: {int(left.sum())} of {self.numel()} output elements were never written"

    def assert_unchanged(self, what=""):
        assert torch.equal(self.ibuf, self.before), f"{what}: an input buffer was modified"

    def assert_untouched(self, what=""):
        """an output slot of a call the host function rejected: still all canary"""
        assert bool((self.ibuf == self.canary).all()), f"{what}: a rejected call wrote to its output"

    def check_output(self, what=""):
        """guards intact and every element written -> the slot as a dense tensor"""
        self.assert_guards_intact(what)
        self.assert_fully_written(what)
        return self.result()


SCRATCH_MODES = ("zeros", "stale", "ones", "nan")
TAIL_BYTES, TAIL_CANARY = 256, 0xC3
_SAME_SIZE_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def canary_of(dtype):
    """(integer view type, value) of the "nan" fill of a dtype: Slot.CANARY's quiet NaNs, a float64 quiet NaN, 0x7F bytes
    for the integer types, True for bool"""
    if dtype in Slot.CANARY:
        return Slot.CANARY[dtype]
    if dtype == torch.float64:
        return torch.int64, 0x7FF80000C0DEBEEF
    if dtype == torch.bool:
        return torch.uint8, 1
    size = dtype.itemsize
    return _SAME_SIZE_INT[size], int.from_bytes(b"\x7f" * size, "little")


def dirty(t, mode):
    """fill tensor `t` (any strides) in place with what `mode` stands for ("zeros" | "ones" | "nan", and "first": 0x5A bytes,
    what a "stale" buffer holds before its first use); -> t"""
    size = t.element_size()
    if size not in _SAME_SIZE_INT:
        raise TypeError(f"no fill for {t.dtype}: elements of 1, 2, 4 or 8 bytes only")
    if t.numel() == 0:
        return t
    with torch.no_grad():
        if mode == "zeros":
            t.view(_SAME_SIZE_INT[size]).zero_()
        elif mode == "ones":
            it = _SAME_SIZE_INT[size]
            t.view(it).fill_(0xFF if it == torch.uint8 else -1)
        elif mode == "nan":
            it, v = canary_of(t.dtype)
            t.view(it).fill_(v)
        elif mode == "first":
            t.view(_SAME_SIZE_INT[size]).fill_(int.from_bytes(b"\x5a" * size, "little"))
        else:
            raise ValueError(mode)
    return t


class Scratch:
    """`with hip.scratch(mode) as s:` -- while active, every workspace and every output the RawOps wrappers allocate holds
    what `mode` says on entry instead of whatever torch.empty returns:

        None     torch.empty (nothing is tracked)
        "zeros"  zeros
        "stale"  the buffer the same call site got last time for the same size (0x5A bytes the first time), not refilled: the call
                 sees what the previous call through that site left.  `s.rewind()` between two runs of the same sequence of
                 calls makes the second run get the first run's buffers, allocation by allocation
        "ones"   every byte 0xFF
        "nan"    canary_of(dtype): quiet-NaN canaries, 0x7F bytes for integers, True for bool; a workspace holds the fp32
                 canary in every word (0x7F bytes where its size is no multiple of 4)

    In every mode but None a workspace is allocated TAIL_BYTES longer than declared, the tail holds TAIL_CANARY and the
    wrapper still passes the declared size; leaving the context checks every tail (AssertionError).  Counters: `workspaces`
    and `outputs` dirtied, `declared` = sum of the workspace bytes the library asked for."""

    _HELPERS = ("_site", "_fresh", "output", "workspace", "empty", "_workspace", "_ws", "_out")

    def __init__(self, ops, mode):
        assert mode is None or mode in SCRATCH_MODES, mode
        self.ops, self.mode = ops, mode
        self.workspaces = self.outputs = self.declared = 0
        self._tails = []            # (whole buffer, declared bytes, site)
        self._stale, self._seen = {}, {}

    def __enter__(self):
        assert self.ops._scratch is None, "scratch() does not nest"
        if self.mode is not None:
            self.ops._scratch = self
        return self

    def __exit__(self, et, ev, tb):
        self.ops._scratch = None
        if et is None:
            self.check_tails()
        return False

    def rewind(self):
        """"stale": the next allocations start over at each call site's first buffer"""
        self._seen.clear()

    def check_tails(self):
        if self.ops.device == "cuda":
            torch.cuda.synchronize()
        for buf, n, site in self._tails:
            bad = (buf[n:] != TAIL_CANARY).nonzero().flatten()
            assert bad.numel() == 0, (f"workspace of {site[0]} (line {site[1]}): {bad.numel()} bytes past the declared {n} were "
                                      f"overwritten, first at +{int(bad[0])}")

    def _site(self):
        f = sys._getframe(0)
        while f.f_code.co_filename == __file__ and f.f_code.co_name in self._HELPERS:
            f = f.f_back
        return f.f_code.co_name, f.f_lineno

    def _fresh(self, kind, nbytes_or_shape, dtype, device, make):
        """the buffer of this allocation: new (and filled), or in "stale" the one this site had for this size before"""
        if self.mode != "stale":
            return make(self.mode)
        key = (kind, self._site(), nbytes_or_shape, dtype)
        k = self._seen.get(key, 0)
        self._seen[key] = k + 1
        if (key, k) not in self._stale:
            self._stale[(key, k)] = make("first")
        return self._stale[(key, k)]

    def output(self, shape, dtype, device):
        self.outputs += 1
        return self._fresh("out", shape, dtype, device,
                           lambda mode: dirty(torch.zeros(shape, dtype=dtype, device=device), mode))

    def workspace(self, n, asked, device):
        self.workspaces += 1
        self.declared += asked
        site = self._site()

        def make(mode):
            buf = torch.zeros(n + TAIL_BYTES, dtype=torch.uint8, device=device)
            assert buf.data_ptr() % 16 == 0
            if mode == "nan" and n % 4 == 0:
                dirty(buf[:n].view(torch.float32), "nan")
            else:
                buf[:n] = {"zeros": 0, "ones": 0xFF, "nan": 0x7F, "first": 0x5A}[mode]
            buf[n:] = TAIL_CANARY
            return buf
        buf = self._fresh("ws", n, torch.uint8, device, make)
        if not any(b is buf for b, _, _ in self._tails):
            self._tails.append((buf, n, site))
        return buf[:n]


def bit_equal(a, b, mask=None):
    """same shape, dtype and bits (NaN payloads and signed zeros included); mask: bool tensor of the defined elements"""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = _SAME_SIZE_INT[a.element_size()]
    ia, ib = a.contiguous().view(it), b.contiguous().view(it)
    if mask is not None:
        ia, ib = ia[mask.to(ia.device)], ib[mask.to(ib.device)]
    return torch.equal(ia, ib)


def assert_recycled(ops, run, other, reference, has_workspace=True, deterministic=True, masks=None, modes=SCRATCH_MODES[1:]):
    """The recycled-memory protocol of one case.  `run()` -> {name: tensor} calls the entry point(s) under test on the
    case's inputs through `ops`, `other()` does the same on other inputs of the same shapes, `reference(got)` asserts
    that a result meets the case's oracle / fp64 reference at its parity test's tolerance.

      (a) two runs on zeroed scratch are bit-identical (asserted unless deterministic=False)
      (b) a run on "stale" (after other()), "ones" and "nan" scratch, in that order, is bit-identical to the clean run in
          every returned tensor (masks: {name: bool tensor of the defined elements} for documented don't-care bytes)
      (c) the "nan" run meets the reference; with deterministic=False every poisoned run does, in place of (b)
      (d) every poisoned run went through at least one dirtied workspace of non-zero declared size (has_workspace; None:
          where the clean run declared one), or else through at least one dirtied output
    Leaving each scratch() checks the workspace tails.  modes: the poisoning modes to run (the harness self-test runs one)."""
    masks = masks or {}
    with ops.scratch("zeros") as s:
        clean = run()
    if has_workspace is None:       # (entry points whose workspace query is 0 on some routes: what the clean run declared)
        has_workspace = s.declared > 0
    with ops.scratch("zeros"):
        again = run()
    if deterministic:
        diff = [k for k in clean if not bit_equal(clean[k], again[k], masks.get(k))]
        assert not diff, f"(a) two runs on zeroed scratch differ in {diff}"
    for mode in modes:
        with ops.scratch(mode) as s:
            if mode == "stale":
                other()
                s.rewind()
            got = run()
        if has_workspace:
            assert s.workspaces >= 1 and s.declared > 0, f"(d) {mode}: {s.workspaces} workspaces of {s.declared} declared bytes"
        else:
            assert s.outputs >= 1, f"(d) {mode}: no output went through the harness"
        if deterministic:
            diff = [k for k in clean if not bit_equal(clean[k], got[k], masks.get(k))]
            assert not diff, f"(b) on {mode!r} scratch {diff} differ from the run on zeroed scratch"
        if mode == "nan" or not deterministic:
            reference(got)


class PoisonedEmpty:
    """`with PoisonedEmpty(monkeypatch, mode) as p:` -- package-level twin of RawOps.scratch for code that allocates through
    torch itself (ops.py): torch.empty, torch.empty_like, torch.empty_strided and Tensor.new_empty are wrapped (pytest's
    monkeypatch, undone on exit, also after an exception) so that every result on a `device_type` device is filled as
    `mode` says ("zeros" | "ones" | "nan"; there is no "stale": call the op once on other inputs first).  CPU and pinned
    tensors are left alone.  torch.zeros / torch.full / tensor.clone are not touched, so whatever the package zero-fills
    (work-queue pool, fp16 overflow word, optimizer state record, caller-zeroed counters) stays as it is.  `p.dirtied`
    counts the allocations filled.  Capture no torch.cuda.graph inside: the fills would be recorded."""

    def __init__(self, monkeypatch, mode, device_type="cuda"):
        assert mode in ("zeros", "ones", "nan"), mode
        self.monkeypatch, self.mode, self.device_type = monkeypatch, mode, device_type
        self.dirtied = 0

    def _wrap(self, orig):
        def wrapped(*a, **k):
            t = orig(*a, **k)
            if (isinstance(t, torch.Tensor) and t.device.type == self.device_type and t.element_size() in _SAME_SIZE_INT
                    and not (t.device.type == "cpu" and t.is_pinned())):      # (16-byte elements: left alone, not counted)
                dirty(t, self.mode)
                self.dirtied += 1
            return t
        return wrapped

    def __enter__(self):
        self._cm = self.monkeypatch.context()
        m = self._cm.__enter__()
        for owner, name in ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty")):
            m.setattr(owner, name, self._wrap(getattr(owner, name)))
        return self

    def __exit__(self, *exc):
        return self._cm.__exit__(*exc)


def _p(t):
    if t is None:
        return None
    return C.c_void_p(t.ptr if isinstance(t, Slot) else t.data_ptr())


def _bs(t, dense=0):
    """batch stride to pass for `t`: a Slot's own, else `dense` (0 = the ABI's "dense")"""
    return t.bs_arg if isinstance(t, Slot) else dense


class RawOps:
    def __init__(self, backend):
        self.backend = backend
        if backend == "hip":
            self.lib, self.prefix, self.device = _lib.lib(), "m355_", "cuda"
        elif backend == "oracle":
            self.lib = _lib.bind(C.CDLL(build_oracle()), prefix="m355o_")
            self.prefix, self.device = "m355o_", "cpu"
        else:
            raise ValueError(backend)
        self._scratch = None

    # ------------------------------------------------------------- plumbing
    def fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream) if self.device == "cuda" else None

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.m355_last_error().decode() if self.backend == "hip" else ""
            raise RuntimeError(f"{what} -> {rc} {msg}")

    def to(self, t):
        if isinstance(t, Slot):
            assert torch.device(t.device).type == self.device
            return t
        return None if t is None else t.to(self.device).contiguous()

    def slot(self, data_or_shape, dtype=torch.float32, **layout):
        """Slot on this backend's device: an input slot holding a tensor, or an output slot of a shape
        (layout: c_pre, c_post, lead, extra -- see Slot)"""
        if isinstance(data_or_shape, torch.Tensor):
            return Slot(self.device, None, data=data_or_shape, **layout)
        return Slot(self.device, tuple(data_or_shape), dtype=dtype, **layout)

    def _out(self, out, shape, dtype=torch.float32, fill=None):
        """the output of a wrapper: the caller's Slot (shape-checked) or a fresh dense tensor"""
        if out is not None:
            assert isinstance(out, Slot) and tuple(out.shape) == tuple(shape) and out.dtype == dtype, (out.shape, shape)
            return out
        if fill is not None and self._scratch is None:
            return torch.full(tuple(shape), fill, dtype=dtype, device=self.device)
        return self.empty(*shape, dtype=dtype)   # (under hip.scratch(mode) the 0.0 / 7.0 pre-fills of c8 outputs become the mode's fill)

    def empty(self, *shape, dtype=torch.float32):
        """every output a wrapper allocates, main or auxiliary: torch.empty, or what the active scratch() mode holds"""
        if self._scratch is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        return self._scratch.output(tuple(shape), dtype, self.device)

    def _workspace(self, nbytes):
        """every workspace a wrapper allocates: `nbytes` from the library's query (at least 16 are handed over).  The tensor's
        numel() is the declared size the wrapper passes; under scratch(mode) it is a view of a buffer with a guarded tail."""
        n = max(int(nbytes), 16)
        if self._scratch is None:
            return torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._scratch.workspace(n, int(nbytes), self.device)

    def _ws(self, qname, desc):
        n = 0
        if self.backend == "hip":
            n = getattr(self.lib, "m355_" + qname)(C.byref(desc))
        return self._workspace(n)

    def scratch(self, mode):
        """Context manager (-> Scratch): what the workspaces and outputs of the wrappers hold on entry while it is active"""
        return Scratch(self, mode)

    # ------------------------------------------------- fp16 overflow word
    def overflow_word(self):
        """Context manager: installs a zeroed int32 device word as the library's overflow word of the current device
        (m355_overflow_flag_set) and yields a reader `take()` -> the word's value, which also clears it.  On exit the
        package's own word (ops._overflow_words) is installed again, or none when it had none -- HIP library only."""
        import contextlib
        from segmentation_pipeline_amd import ops
        assert self.backend == "hip"
        lib = self.lib

        @contextlib.contextmanager
        def cm():
            idx = torch.cuda.current_device()
            word = torch.zeros(1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            self._chk(lib.m355_overflow_flag_set(_p(word), idx), "overflow_flag_set")

            def take():
                torch.cuda.synchronize()
                v = int(word.item())
                word.zero_()
                return v
            try:
                yield take
            finally:
                torch.cuda.synchronize()
                prev = ops._overflow_words.get(idx)
                self._chk(lib.m355_overflow_flag_set(_p(prev), idx), "overflow_flag_set(restore)")
        return cm()

    # ------------------------------------------------------------------ conv
    @staticmethod
    def conv_desc(x_shape, Cout, k, stride, pad, out_pad=0, xbs=0, ybs=0, compute=0):
        N, Cin, D, H, W = x_shape
        return ConvDesc(N, Cin, Cout, D, H, W, k, stride, pad, out_pad, xbs, ybs, compute, 0)

    def pack_weights(self, w, x_shape, which, compute=0):
        """m355_conv3d_pack: (packed buffer, descriptor flags) -- HIP library only"""
        w = self.to(w)
        d = self.conv_desc(x_shape, w.shape[0], w.shape[2], 1, 1, compute=compute)
        n = self.lib.m355_conv3d_packed_bytes(C.byref(d), which)
        assert n > 0
        buf = torch.full((int(n),), 0xA5, dtype=torch.uint8, device=self.device)   # (bytes a layout leaves unwritten compare equal)
        self._chk(self.lib.m355_conv3d_pack(C.byref(d), which, _p(w), _p(buf), self._stream()), "conv3d_pack")
        return buf

    def pack_weights_batch(self, cases):
        """m355_conv3d_pack_batch over cases [(w, x_shape, which, compute)] -> list of packed buffers"""
        items, bufs, keep = [], [], []
        for w, x_shape, which, compute in cases:
            w = self.to(w)
            d = self.conv_desc(x_shape, w.shape[0], w.shape[2], 1, 1, compute=compute)
            n = self.lib.m355_conv3d_packed_bytes(C.byref(d), which)
            assert n > 0
            buf = torch.full((int(n),), 0xA5, dtype=torch.uint8, device=self.device)
            items.append(_lib.PackItem(d, which, w.data_ptr(), buf.data_ptr()))
            bufs.append(buf)
            keep.append(w)
        arr = (_lib.PackItem * len(items))(*items)
        self._chk(self.lib.m355_conv3d_pack_batch(C.cast(arr, C.c_void_p), len(items), self._stream()), "conv3d_pack_batch")
        torch.cuda.synchronize()
        return bufs

    def conv3d_fwd(self, x, w, bias=None, add=None, stride=1, pad=1, compute=0, packed=None, softmax=False, out=None):
        """packed: buffer from pack_weights(w, x.shape, 0) -> the call uses M355_CONV_W_PACKED;
        softmax: M355_CONV_SOFTMAX (HIP library, descriptors with m355_conv3d_fuses_softmax != 0);
        x / add: tensors or Slots, out: an output Slot (returned) -- `add` shares y's batch stride"""
        x, w, bias, add = map(self.to, (x, w, bias, add))
        k = w.shape[2]
        od = lambda n: (n + 2 * pad - k) // stride + 1
        y = self._out(out, (x.shape[0], w.shape[0], od(x.shape[2]), od(x.shape[3]), od(x.shape[4])))
        assert _bs(add, _bs(y)) == _bs(y) and (add is None or isinstance(add, Slot) == isinstance(y, Slot) or x.shape[0] == 1)
        d = self.conv_desc(x.shape, w.shape[0], k, stride, pad, xbs=_bs(x), ybs=_bs(y), compute=compute)
        if softmax:
            assert self.lib.m355_conv3d_fuses_softmax(C.byref(d)) == 1
            d.flags |= _lib.CONV_SOFTMAX
        if packed is not None:
            d.flags = _lib.CONV_W_PACKED
            ws = self._ws("conv3d_fwd_workspace", d)
            self._chk(self.fn("conv3d_fwd")(C.byref(d), _p(x), _p(packed), _p(bias), _p(add), _p(y), _p(ws), ws.numel(),
                                            self._stream()), "conv3d_fwd(packed)")
            return y
        ws = self._ws("conv3d_fwd_workspace", d)
        self._chk(self.fn("conv3d_fwd")(C.byref(d), _p(x), _p(w), _p(bias), _p(add), _p(y), _p(ws), ws.numel(),
                                        self._stream()), "conv3d_fwd")
        return y

    # ---- c8 tensors of the 16-bit compute modes (HIP library only; dtype: 1 = bf16, 2 = fp16) ----
    @staticmethod
    def dt16(compute):
        return torch.bfloat16 if compute == 1 else torch.float16

    def act16_pack(self, x, compute, pad_batch=0, out=None):
        """fp32 [N,C,D,H,W] -> c8 tensor (torch 16-bit dtype, shape [N, CB (+pad), S, 8]); pad_batch > 0 leaves
        that many unused channel blocks per sample (a non-dense batch stride).  x: tensor or Slot; out: a c8 Slot."""
        x = self.to(x)
        N, Cc = x.shape[:2]
        S = x.numel() // (N * Cc)
        CB = (Cc + 7) // 8
        dt = self.dt16(compute)
        x16 = self._out(out, (N, CB + pad_batch, S, 8), dt, fill=7.0)
        self._chk(self.fn("act16_pack")(_p(x), _p(x16), N, Cc, S, _bs(x), _bs(x16, (CB + pad_batch) * S * 8), compute,
                                        self._stream()), "act16_pack")
        return x16

    def act16_unpack(self, x16, Cc, spatial, compute, out=None):
        N, CBp, S, _ = x16.shape
        x = self._out(out, (N, Cc) + tuple(spatial))
        self._chk(self.fn("act16_unpack")(_p(x16), _p(x), N, Cc, S, _bs(x16, CBp * S * 8), _bs(x), compute, self._stream()),
                  "act16_unpack")
        return x

    def conv_plan(self, x_shape, Cout, compute=0, which=0, xbs=0, ybs=0):
        """(kernel family, NTW, GX, split-K) of the 3x3x3 kernel the library picks (m355_conv3d_plan)"""
        d = self.conv_desc(x_shape, Cout, 3, 1, 1, xbs=xbs, ybs=ybs, compute=compute)
        out = (C.c_int32 * 4)()
        self._chk(self.lib.m355_conv3d_plan(C.byref(d), which, out), "conv3d_plan")
        return tuple(out)

    def conv_launch_plan(self, entry, x_shape, Cout, compute=0, flags=0, tensors=(), strides=(0, 0), workspace_bytes=1 << 40,
                         xbs=0, ybs=0, k=3, stride=1, pad=1):
        """the twelve numbers of m355_conv3d_launch_plan (variant, grid x / y / z, block, 16-row grid x / z, auxiliary launches,
        workspace bytes, reduction grid, two workspace offsets) for a call of entry point _lib.CONV_ENTRIES[entry].  tensors:
        up to seven Slot / torch tensor / integer address / None in the query's pointer order (first operand, w | second
        operand, bias | fp32 dy, add, output, statistics | dbias, workspace); missing first operand, w, output and workspace
        default to aligned dummies"""
        addr = lambda t: 0 if t is None else (t if isinstance(t, int) else (t.ptr if isinstance(t, Slot) else t.data_ptr()))   # noqa: E731
        ptrs = [addr(t) for t in tensors] + [0] * (7 - len(tensors))
        for i in (0, 1, 4, 6):
            ptrs[i] = ptrs[i] or 4096 * (i + 1)
        d = self.conv_desc(x_shape, Cout, k, stride, pad, xbs=xbs, ybs=ybs, compute=compute)
        d.flags = flags
        out = (C.c_int64 * 12)()
        self._chk(self.lib.m355_conv3d_launch_plan(entry, C.byref(d), (C.c_int64 * 2)(*strides), (C.c_uint64 * 7)(*ptrs),
                                                   workspace_bytes, out), "conv3d_launch_plan")
        return tuple(out)

    def convt_plan(self, x_shape, Cout, k=2, stride=2, pad=0, out_pad=0, compute=0, which=0, xbs=0, ybs=0, y_side=None):
        """(kernel family, three numbers of its launch) of a conv-transpose call (m355_conv_transpose3d_plan; which 0..2 the
        fp32 entry points, 3..5 the c8 ones).  y_side: the y / dy tensor or Slot the call would get (None: aligned)"""
        d = self.conv_desc(x_shape, Cout, k, stride, pad, out_pad, xbs=xbs, ybs=ybs, compute=compute)
        out = (C.c_int32 * 4)()
        self._chk(self.lib.m355_conv_transpose3d_plan(C.byref(d), which, _p(y_side), out), "conv_transpose3d_plan")
        return tuple(out)

    def resample_plan(self, op, shape, tensors, routes=None, compute=0):
        """(variant, grid x, y, z, LDS bytes, three resolved batch strides) of a call of the resampling family
        (m355_resample_plan).  op: index into _lib.RESAMPLE_OPS; shape: (N, C, D, H, W) as that entry point takes them;
        tensors: its tensors in the order of its batch strides -- Slot, torch tensor (dense) or None; routes: the max-pool
        route tensor"""
        addr = lambda t: 0 if t is None else (t.ptr if isinstance(t, Slot) else t.data_ptr())   # noqa: E731
        tensors = list(tensors) + [None] * (3 - len(tensors))
        strides = (C.c_int64 * 3)(*[0 if t is None else _bs(t) for t in tensors])
        pointers = (C.c_uint64 * 4)(*[addr(t) for t in tensors], addr(routes))
        out = (C.c_int64 * 8)()
        self._chk(self.lib.m355_resample_plan(op, *shape, strides, pointers, compute, out), "resample_plan")
        return tuple(out)

    def conv3d_fwd_h16(self, x16, Cin, spatial, w, bias=None, add=None, compute=1, groups=None, eps=1e-5, softmax=False,
                       out=None, partials=False):
        """forward on a c8 input; groups != None also returns the fused statistics (mean, rstd); softmax: the
        M355_CONV_SOFTMAX epilogue (asserts that the library offers it for this descriptor)"""
        w, bias, add = map(self.to, (w, bias, add))
        N, CBp, S, _ = x16.shape
        Cout = w.shape[0]
        y = self._out(out, (N, Cout) + tuple(spatial))
        assert add is None or _bs(add) == _bs(y)
        d = self.conv_desc((N, Cin) + tuple(spatial), Cout, 3, 1, 1, ybs=_bs(y), compute=compute)
        if softmax:
            assert self.lib.m355_conv3d_fuses_softmax(C.byref(d)) == 1
            d.flags |= 2
        n = self.lib.m355_conv3d_h16_workspace(C.byref(d), 0)
        ws = self._workspace(n)
        part = None
        if groups is not None:
            slots = self.fn("conv3d_stats_slots")(C.byref(d))
            assert slots > 0
            part = self.empty(N, slots, Cout, 2)
        self._chk(self.fn("conv3d_fwd_h16")(C.byref(d), _p(x16), _bs(x16, CBp * S * 8), _p(w), _p(bias), _p(add), _p(y), _p(part),
                                            _p(ws), ws.numel(), self._stream()), "conv3d_fwd_h16")
        if groups is None:
            return y
        nd = NormDesc(N, Cout, S, groups, 0, eps, 0.01, 0, 0, 0)
        ns = self.fn("norm_num_stats")(C.byref(nd))
        mean, rstd = self.empty(ns), self.empty(ns)
        nws = self._ws("norm_workspace", nd)
        self._chk(self.fn("norm_stats_from_partials")(C.byref(nd), _p(part), slots, _p(mean), _p(rstd), None, None,
                                                      0.1, _p(nws), nws.numel(), self._stream()),
                  "norm_stats_from_partials")
        return (y, mean, rstd, part) if partials else (y, mean, rstd)

    def conv3d_fwd_h16_c8(self, x16, Cin, spatial, w, bias=None, compute=1, with_stats=False, out=None):
        """forward with c8 input AND c8 output; with_stats -> (y16, partials [N, P, Cout, 2])"""
        w, bias = self.to(w), self.to(bias)
        N, CBp, S, _ = x16.shape
        Cout = w.shape[0]
        d = self.conv_desc((N, Cin) + tuple(spatial), Cout, 3, 1, 1, compute=compute)
        y16 = self._out(out, (N, (Cout + 7) // 8, S, 8), x16.dtype, fill=0.0)
        n = self.lib.m355_conv3d_h16_workspace(C.byref(d), 0)
        ws = self._workspace(n)
        part = None
        if with_stats:
            slots = self.fn("conv3d_stats_slots_c8")(C.byref(d))
            assert slots > 0
            part = self.empty(N, slots, Cout, 2)
        self._chk(self.fn("conv3d_fwd_h16_c8")(C.byref(d), _p(x16), _bs(x16, CBp * S * 8), _p(w), _p(bias), _p(y16), _bs(y16), _p(part),
                                               _p(ws), ws.numel(), self._stream()), "conv3d_fwd_h16_c8")
        return (y16, part) if with_stats else y16

    def norm_act_fwd_c8(self, x16, Cc, mean, rstd, gamma, beta, groups, act, compute, add16=None, eps=1e-5, slope=0.01,
                        out=None):
        mean, rstd, gamma, beta = map(self.to, (mean, rstd, gamma, beta))
        N, CB, S, _ = x16.shape
        d = NormDesc(N, Cc, S, groups, act, eps, slope, 0, 0, 0)
        y16 = self._out(out, x16.shape, x16.dtype)
        self._chk(self.fn("norm_act_fwd_c8")(C.byref(d), _p(x16), _bs(x16), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(add16),
                                             _bs(add16), _p(y16), _bs(y16), compute, self._stream()), "norm_act_fwd_c8")
        return y16

    def act16_channel_partials(self, x16, Cc, compute):
        N, CB, S, _ = x16.shape
        slots = int(self.lib.m355_act16_partials_slots(S))
        part = self.empty(N, slots, Cc, 2)
        self._chk(self.fn("act16_channel_partials")(_p(x16), _bs(x16), N, Cc, S, compute, _p(part), self._stream()),
                  "act16_channel_partials")
        return part

    def conv3d_bwd_data_h16(self, dy16, Cout, w, x_shape, compute=1, out=None):
        w = self.to(w)
        N, CBp, S, _ = dy16.shape
        dx = self._out(out, x_shape)
        d = self.conv_desc(x_shape, Cout, 3, 1, 1, xbs=_bs(dx), compute=compute)
        n = self.lib.m355_conv3d_h16_workspace(C.byref(d), 1)
        ws = self._workspace(n)
        self._chk(self.fn("conv3d_bwd_data_h16")(C.byref(d), _p(dy16), _bs(dy16, CBp * S * 8), _p(w), _p(dx), _p(ws), ws.numel(),
                                                 self._stream()), "conv3d_bwd_data_h16")
        return dx

    def conv3d_bwd_weight_h16(self, x16, dy16, dy, Cin, Cout, spatial, compute=1, with_bias=True):
        """weight (and bias) gradient of the 3x3x3 conv from c8 operands"""
        N = x16.shape[0]
        d = self.conv_desc((N, Cin) + tuple(spatial), Cout, 3, 1, 1, compute=compute)
        dw, db = self.empty(Cout, Cin, 3, 3, 3), (self.empty(Cout) if with_bias else None)
        n = self.lib.m355_conv3d_bwd_weight_h16_workspace(C.byref(d))
        ws = self._workspace(n)
        d.y_batch_stride = _bs(dy) if with_bias else 0
        self._chk(self.fn("conv3d_bwd_weight_h16")(C.byref(d), _p(x16), _bs(x16), _p(dy16), _bs(dy16), _p(self.to(dy)) if with_bias else None,
                                                   _p(dw), _p(db), _p(ws), ws.numel(), self._stream()),
                  "conv3d_bwd_weight_h16")
        return dw, db

    def conv_transpose3d_fwd_h16(self, x16, Cin, spatial, w, bias, compute, out=None):
        """k2 s2 conv-transpose c8 -> c8; returns the c8 output [N, CBout, 8S, 8]"""
        w, bias = self.to(w), self.to(bias)
        N, CB, S, _ = x16.shape
        Cout = w.shape[1]
        d = self.conv_desc((N, Cin) + tuple(spatial), Cout, 2, 2, 0)
        y16 = self._out(out, (N, (Cout + 7) // 8, 8 * S, 8), x16.dtype)
        self._chk(self.fn("conv_transpose3d_fwd_h16")(C.byref(d), _p(x16), _bs(x16), _p(w), _p(bias), _p(y16), _bs(y16), compute,
                                                      self._stream()), "conv_transpose3d_fwd_h16")
        return y16

    # ---- c8-only training flow (round 3) ----
    def act16_pack_scaled(self, x, compute, scale, out=None):
        x = self.to(x)
        N, Cc = x.shape[:2]
        S = x.numel() // (N * Cc)
        x16 = self._out(out, (N, (Cc + 7) // 8, S, 8), self.dt16(compute), fill=7.0)
        self._chk(self.fn("act16_pack_scaled")(_p(x), _p(x16), N, Cc, S, _bs(x), _bs(x16), compute, float(scale),
                                               self._stream()), "act16_pack_scaled")
        return x16

    def act16_unpack_scaled(self, x16, Cc, spatial, compute, scale, out=None):
        N, CBp, S, _ = x16.shape
        x = self._out(out, (N, Cc) + tuple(spatial))
        self._chk(self.fn("act16_unpack_scaled")(_p(x16), _p(x), N, Cc, S, _bs(x16, CBp * S * 8), _bs(x), compute,
                                                 float(scale), self._stream()), "act16_unpack_scaled")
        return x

    def conv3d_bwd_data_h16_c8(self, dy16, Cout, w, x_shape, compute=1, out=None):
        w = self.to(w)
        N, CBp, S, _ = dy16.shape
        d = self.conv_desc(x_shape, Cout, 3, 1, 1, compute=compute)
        dx16 = self._out(out, (N, (x_shape[1] + 7) // 8, S, 8), dy16.dtype, fill=7.0)
        n = self.lib.m355_conv3d_h16_workspace(C.byref(d), 1)
        ws = self._workspace(n)
        self._chk(self.fn("conv3d_bwd_data_h16_c8")(C.byref(d), _p(dy16), _bs(dy16, CBp * S * 8), _p(w), _p(dx16), _bs(dx16), _p(ws), ws.numel(),
                                                    self._stream()), "conv3d_bwd_data_h16_c8")
        return dx16

    def conv3d_bwd_weight_c8(self, x16, dy16, Cin, Cout, spatial, compute=1, with_bias=True, unscale=1.0):
        N = x16.shape[0]
        d = self.conv_desc((N, Cin) + tuple(spatial), Cout, 3, 1, 1, compute=compute)
        dw, db = self.empty(Cout, Cin, 3, 3, 3), (self.empty(Cout) if with_bias else None)
        n = self.lib.m355_conv3d_bwd_weight_c8_workspace(C.byref(d))
        ws = self._workspace(n)
        self._chk(self.fn("conv3d_bwd_weight_c8")(C.byref(d), _p(x16), _bs(x16), _p(dy16), _bs(dy16), _p(dw), _p(db), float(unscale), _p(ws),
                                                  ws.numel(), self._stream()), "conv3d_bwd_weight_c8")
        return dw, db

    def norm_act_bwd_c8(self, x16, dy16, dpool16, Cc, spatial, mean, rstd, gamma, beta, groups, act, compute, training=1,
                        unscale=1.0, eps=1e-5, slope=0.01, out=None):
        """-> (dx16, dgamma, dbeta); dy16 / dpool16: c8 gradients (either may be None, not both)"""
        mean, rstd, gamma, beta = map(self.to, (mean, rstd, gamma, beta))
        N, S = x16.shape[0], x16.shape[2]
        D, H, W = spatial
        d = NormDesc(N, Cc, S, groups, act, eps, slope, 0, 0, 0)
        dx16 = self._out(out, x16.shape, x16.dtype, fill=7.0)
        dg = self.empty(Cc) if gamma is not None else None
        db = self.empty(Cc) if gamma is not None else None
        ws = self._ws("norm_workspace", d)
        self._chk(self.fn("norm_act_bwd_c8")(C.byref(d), _p(x16), _bs(x16), _p(dy16), _bs(dy16), _p(dpool16), _bs(dpool16), D, H, W,
                                             _p(mean), _p(rstd),
                                             _p(gamma), _p(beta), _p(dx16), _bs(dx16), _p(dg), _p(db), training, float(unscale),
                                             compute, _p(ws), ws.numel(), self._stream()), "norm_act_bwd_c8")
        return dx16, dg, db

    def avgpool_bwd_h16(self, dpool16, dskip16, Cc, spatial, compute, out=None):
        D, H, W = spatial
        N = dpool16.shape[0]
        dx16 = self._out(out, (N, (Cc + 7) // 8, D * H * W, 8), dpool16.dtype, fill=7.0)
        self._chk(self.fn("avgpool3d_2x_bwd_h16")(_p(dpool16), _p(dskip16), _p(dx16), N, Cc, D, H, W, _bs(dpool16), _bs(dskip16),
                                                  _bs(dx16), compute,
                                                  self._stream()), "avgpool3d_2x_bwd_h16")
        return dx16

    def upsample_trilinear2x_fwd_h16(self, x16, Cc, spatial, compute, pad_batch=0, out=None):
        """c8 -> c8 at twice the resolution; pad_batch: unused channel blocks per sample of the destination"""
        D, H, W = spatial
        N, CBp = x16.shape[:2]
        CB = (Cc + 7) // 8
        y16 = self._out(out, (N, CB + pad_batch, 8 * D * H * W, 8), x16.dtype, fill=7.0)
        self._chk(self.fn("upsample_trilinear2x_fwd_h16")(_p(x16), _p(y16), N, Cc, D, H, W, _bs(x16, CBp * D * H * W * 8),
                                                          _bs(y16, (CB + pad_batch) * D * H * W * 64), compute, self._stream()),
                  "upsample_trilinear2x_fwd_h16")
        return y16

    def upsample_trilinear2x_bwd_h16(self, dy16, Cc, spatial, compute, out=None):
        """`spatial`: the LOW-resolution size"""
        D, H, W = spatial
        N, CBp = dy16.shape[:2]
        dx16 = self._out(out, (N, (Cc + 7) // 8, D * H * W, 8), dy16.dtype, fill=7.0)
        self._chk(self.fn("upsample_trilinear2x_bwd_h16")(_p(dy16), _p(dx16), N, Cc, D, H, W, _bs(dy16, CBp * D * H * W * 64),
                                                          _bs(dx16), compute, self._stream()), "upsample_trilinear2x_bwd_h16")
        return dx16

    def act16_channel_scale(self, x16, scale, Cc, compute, out=None):
        scale = self.to(scale)
        N, CBp, S, _ = x16.shape
        y16 = self._out(out, (N, (Cc + 7) // 8, S, 8), x16.dtype, fill=7.0)
        self._chk(self.fn("act16_channel_scale")(_p(x16), _p(scale), _p(y16), N, Cc, S, _bs(x16, CBp * S * 8), _bs(y16), compute,
                                                 self._stream()), "act16_channel_scale")
        return y16

    def s2d_h16(self, x16, full_shape, compute, to_depth, pad_batch=0, out=None):
        """space-to-depth (to_depth) / depth-to-space by 2, c8 -> c8; `full_shape` = (N, C, D, H, W) of the full-resolution
        tensor; pad_batch: unused channel blocks per sample of the destination"""
        N, Cc, D, H, W = full_shape
        S = D * H * W
        CBp = x16.shape[1]
        if to_depth:
            y16 = self._out(out, (N, Cc + pad_batch, S // 8, 8), x16.dtype, fill=7.0)
            xbs, ybs = _bs(x16, CBp * S * 8), _bs(y16, (Cc + pad_batch) * (S // 8) * 8)
            fn = self.fn("space_to_depth2_h16")
        else:
            CB = (Cc + 7) // 8
            y16 = self._out(out, (N, CB + pad_batch, S, 8), x16.dtype, fill=7.0)
            xbs, ybs = _bs(x16, CBp * (S // 8) * 8), _bs(y16, (CB + pad_batch) * S * 8)
            fn = self.fn("depth_to_space2_h16")
        self._chk(fn(_p(x16), _p(y16), N, Cc, D, H, W, xbs, ybs, compute, self._stream()), "s2d_h16")
        return y16

    def convt_h16_bwd_supported(self, x_shape, Cout):
        d = self.conv_desc(x_shape, Cout, 2, 2, 0)
        return bool(self.lib.m355_conv_transpose3d_h16_bwd_supported(C.byref(d)))

    def convt_bwd_data_h16(self, dy16, w, x_shape, compute, out=None):
        w = self.to(w)
        N, Cin = x_shape[:2]
        S = x_shape[2] * x_shape[3] * x_shape[4]
        d = self.conv_desc(x_shape, w.shape[1], 2, 2, 0)
        dx16 = self._out(out, (N, (Cin + 7) // 8, S, 8), dy16.dtype, fill=7.0)
        self._chk(self.fn("conv_transpose3d_bwd_data_h16")(C.byref(d), _p(dy16), _bs(dy16), _p(w), _p(dx16), _bs(dx16), compute,
                                                           self._stream()), "conv_transpose3d_bwd_data_h16")
        return dx16

    def convt_bwd_weight_h16(self, x16, dy16, x_shape, Cout, compute, with_bias=True, unscale=1.0):
        d = self.conv_desc(x_shape, Cout, 2, 2, 0)
        dw = self.empty(x_shape[1], Cout, 2, 2, 2)
        db = self.empty(Cout) if with_bias else None
        n = self.lib.m355_conv_transpose3d_h16_bwd_workspace(C.byref(d))
        ws = self._workspace(n)
        self._chk(self.fn("conv_transpose3d_bwd_weight_h16")(C.byref(d), _p(x16), _bs(x16), _p(dy16), _bs(dy16), _p(dw), _p(db), float(unscale),
                                                             compute, _p(ws), ws.numel(), self._stream()),
                  "conv_transpose3d_bwd_weight_h16")
        return dw, db

    def conv3d_fwd_stats(self, x, w, bias=None, groups=0, eps=1e-5, compute=0, out=None, partials=False):
        """fused conv + statistics: returns (y, mean, rstd) of the normalisation that follows the conv, or
        None when this backend has no fused statistics for the shape; partials: (y, mean, rstd, partials [N, P, Cout, 2])"""
        x, w = self.to(x), self.to(w)
        bias = self.to(bias) if bias is not None else None
        N, Cin, D, H, W = x.shape
        Cout = w.shape[0]
        y = self._out(out, (N, Cout, D, H, W))
        d = self.conv_desc(x.shape, Cout, 3, 1, 1, xbs=_bs(x), ybs=_bs(y), compute=compute)
        slots = self.fn("conv3d_stats_slots")(C.byref(d))
        if slots <= 0:
            return None
        part = self.empty(N, slots, Cout, 2)
        ws = self._ws("conv3d_fwd_workspace", d)
        self._chk(self.fn("conv3d_fwd_stats")(C.byref(d), _p(x), _p(w), _p(bias), None, _p(y), _p(part), _p(ws),
                                              ws.numel(), self._stream()), "conv3d_fwd_stats")
        nd = NormDesc(N, Cout, D * H * W, groups, 0, eps, 0.01, 0, 0, 0)
        ns = self.fn("norm_num_stats")(C.byref(nd))
        mean, rstd = self.empty(ns), self.empty(ns)
        nws = self._ws("norm_workspace", nd)
        self._chk(self.fn("norm_stats_from_partials")(C.byref(nd), _p(part), slots, _p(mean), _p(rstd), None, None,
                                                      0.1, _p(nws), nws.numel(), self._stream()),
                  "norm_stats_from_partials")
        return (y, mean, rstd, part) if partials else (y, mean, rstd)

    def norm_stats_from_partials(self, part, x_shape, groups, eps=1e-5):
        """(mean, rstd) from the partials [N, P, C, 2] of a conv epilogue or of act16_channel_partials"""
        part = self.to(part)
        N, Cc = x_shape[:2]
        nd = NormDesc(N, Cc, torch.Size(x_shape).numel() // (N * Cc), groups, 0, eps, 0.01, 0, 0, 0)
        ns = self.fn("norm_num_stats")(C.byref(nd))
        mean, rstd = self.empty(ns), self.empty(ns)
        nws = self._ws("norm_workspace", nd)
        self._chk(self.fn("norm_stats_from_partials")(C.byref(nd), _p(part), part.shape[1], _p(mean), _p(rstd), None, None,
                                                      0.1, _p(nws), nws.numel(), self._stream()), "norm_stats_from_partials")
        return mean, rstd

    def conv3d_bwd_data(self, dy, w, x_shape, stride=1, pad=1, compute=0, packed=None, out=None):
        dy, w = self.to(dy), self.to(w)
        dx = self._out(out, x_shape)
        d = self.conv_desc(x_shape, w.shape[0], w.shape[2], stride, pad, xbs=_bs(dx), ybs=_bs(dy), compute=compute)
        ws = self._ws("conv3d_bwd_data_workspace", d)
        if packed is not None:
            d.flags, w = _lib.CONV_W_PACKED, packed
        self._chk(self.fn("conv3d_bwd_data")(C.byref(d), _p(dy), _p(w), _p(dx), _p(ws), ws.numel(), self._stream()),
                  "conv3d_bwd_data")
        return dx

    def conv3d_bwd_weight(self, x, dy, k, stride=1, pad=1, with_bias=True, compute=0):
        x, dy = self.to(x), self.to(dy)
        Cout = dy.shape[1]
        d = self.conv_desc(x.shape, Cout, k, stride, pad, xbs=_bs(x), ybs=_bs(dy), compute=compute)
        dw = self.empty(Cout, x.shape[1], k, k, k)
        db = self.empty(Cout) if with_bias else None
        ws = self._ws("conv3d_bwd_weight_workspace", d)
        self._chk(self.fn("conv3d_bwd_weight")(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _p(ws), ws.numel(),
                                               self._stream()), "conv3d_bwd_weight")
        return dw, db

    def convt_fwd(self, x, w, bias=None, stride=2, pad=0, out_pad=0, compute=0, out=None):
        x, w, bias = map(self.to, (x, w, bias))
        k = w.shape[2]
        od = lambda n: (n - 1) * stride - 2 * pad + k + out_pad
        y = self._out(out, (x.shape[0], w.shape[1], od(x.shape[2]), od(x.shape[3]), od(x.shape[4])))
        d = self.conv_desc(x.shape, w.shape[1], k, stride, pad, out_pad, xbs=_bs(x), ybs=_bs(y), compute=compute)
        ws = self._ws("conv_transpose3d_workspace", d)
        self._chk(self.fn("conv_transpose3d_fwd")(C.byref(d), _p(x), _p(w), _p(bias), _p(y), _p(ws), ws.numel(),
                                                  self._stream()), "convt_fwd")
        return y

    def convt_bwd_data(self, dy, w, x_shape, stride=2, pad=0, out_pad=0, out=None):
        dy, w = self.to(dy), self.to(w)
        dx = self._out(out, x_shape)
        d = self.conv_desc(x_shape, w.shape[1], w.shape[2], stride, pad, out_pad, xbs=_bs(dx), ybs=_bs(dy))
        ws = self._ws("conv_transpose3d_workspace", d)
        self._chk(self.fn("conv_transpose3d_bwd_data")(C.byref(d), _p(dy), _p(w), _p(dx), _p(ws), ws.numel(),
                                                       self._stream()), "convt_bwd_data")
        return dx

    def convt_bwd_weight(self, x, dy, k, stride=2, pad=0, out_pad=0, with_bias=True):
        x, dy = self.to(x), self.to(dy)
        Cout = dy.shape[1]
        d = self.conv_desc(x.shape, Cout, k, stride, pad, out_pad, xbs=_bs(x), ybs=_bs(dy))
        dw = self.empty(x.shape[1], Cout, k, k, k)
        db = self.empty(Cout) if with_bias else None
        ws = self._ws("conv_transpose3d_workspace", d)
        self._chk(self.fn("conv_transpose3d_bwd_weight")(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _p(ws),
                                                         ws.numel(), self._stream()), "convt_bwd_weight")
        return dw, db

    def convt_bwd_weight_x3(self, x, dy, with_bias=True):
        """m355_conv_transpose3d_bwd_weight_x3 (k2 s2, the split pipe) on dense tensors -> (dw, dbias, voxel-range splits of
        the plan); asserts that the library has the split kernel for the descriptor -- HIP library only"""
        x, dy = self.to(x), self.to(dy)
        Cout = dy.shape[1]
        d = self.conv_desc(x.shape, Cout, 2, 2, 0, compute=3)
        plan = (C.c_int32 * 4)()
        self._chk(self.lib.m355_conv_transpose3d_x3_bwd_plan(C.byref(d), 2, _p(dy), plan), "conv_transpose3d_x3_bwd_plan")
        assert plan[0] == 2 and self.lib.m355_conv_transpose3d_x3_bwd_supported(C.byref(d), _p(dy)) == 2, tuple(plan)
        dw = self.empty(x.shape[1], Cout, 2, 2, 2)
        db = self.empty(Cout) if with_bias else None
        ws = self._workspace(self.lib.m355_conv_transpose3d_x3_bwd_workspace(C.byref(d)))
        self._chk(self.lib.m355_conv_transpose3d_bwd_weight_x3(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _p(ws), ws.numel(),
                                                               self._stream()), "conv_transpose3d_bwd_weight_x3")
        return dw, db, plan[2]

    # ------------------------------------------------------------------ norm
    @staticmethod
    def norm_desc(x, groups, act=0, eps=1e-5, slope=0.01, xbs=0, ybs=0, abs_=0):
        N, Cc = x.shape[:2]
        S = x.numel() // (N * Cc)
        return NormDesc(N, Cc, S, groups, act, eps, slope, xbs, ybs, abs_)

    def norm_stats(self, x, groups, eps=1e-5, running=None, momentum=0.1):
        x = self.to(x)
        d = self.norm_desc(x, groups, eps=eps, xbs=_bs(x))
        ns = self.fn("norm_num_stats")(C.byref(d))
        mean, rstd = self.empty(ns), self.empty(ns)
        rm = rv = None
        if running is not None:
            rm, rv = self.to(running[0]).clone(), self.to(running[1]).clone()
        ws = self._ws("norm_workspace", d)
        self._chk(self.fn("norm_stats")(C.byref(d), _p(x), _p(mean), _p(rstd), _p(rm), _p(rv), momentum, _p(ws),
                                        ws.numel(), self._stream()), "norm_stats")
        return mean, rstd, rm, rv

    def norm_act_fwd(self, x, mean, rstd, gamma, beta, groups, act, add=None, eps=1e-5, slope=0.01, out=None):
        x, mean, rstd, gamma, beta, add = map(self.to, (x, mean, rstd, gamma, beta, add))
        y = self._out(out, x.shape)
        d = self.norm_desc(x, groups, act, eps, slope, _bs(x), _bs(y), _bs(add))
        self._chk(self.fn("norm_act_fwd")(C.byref(d), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(add),
                                          _p(y), self._stream()), "norm_act_fwd")
        return y

    def norm_act_fwd_h16(self, x, mean, rstd, gamma, beta, groups, act, compute, add=None, want_f32=False, eps=1e-5,
                         slope=0.01, out16=None, out=None):
        """c8 output (torch 16-bit tensor [N, CB, S, 8]) and optionally the fp32 NCDHW output as well"""
        x, mean, rstd, gamma, beta, add = map(self.to, (x, mean, rstd, gamma, beta, add))
        N, Cc = x.shape[:2]
        S = x.numel() // (N * Cc)
        y16 = self._out(out16, (N, (Cc + 7) // 8, S, 8), self.dt16(compute))
        y = self._out(out, x.shape) if (want_f32 or out is not None) else None
        d = self.norm_desc(x, groups, act, eps, slope, _bs(x), _bs(y), _bs(add))
        self._chk(self.fn("norm_act_fwd_h16")(C.byref(d), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(add), _p(y),
                                              _p(y16), _bs(y16), compute, self._stream()), "norm_act_fwd_h16")
        return y16, y

    def avgpool_fwd_h16(self, x16, Cc, spatial, compute, out=None):
        N, CB, S, _ = x16.shape
        D, H, W = spatial
        y16 = self._out(out, (N, CB, S // 8, 8), x16.dtype)
        self._chk(self.fn("avgpool3d_2x_fwd_h16")(_p(x16), _p(y16), N, Cc, D, H, W, _bs(x16), _bs(y16), compute, self._stream()),
                  "avgpool3d_2x_fwd_h16")
        return y16

    def norm_act_bwd(self, x, dy, mean, rstd, gamma, beta, groups, act, training=1, eps=1e-5, slope=0.01, out=None):
        """x and dx share desc.x_batch_stride, dy has desc.y_batch_stride"""
        x, dy, mean, rstd, gamma, beta = map(self.to, (x, dy, mean, rstd, gamma, beta))
        dx = self._out(out, x.shape)
        assert _bs(dx) == _bs(x) or x.shape[0] == 1
        d = self.norm_desc(x, groups, act, eps, slope, _bs(x), _bs(dy))
        dg = self.empty(x.shape[1]) if gamma is not None else None
        db = self.empty(x.shape[1]) if gamma is not None else None
        ws = self._ws("norm_workspace", d)
        self._chk(self.fn("norm_act_bwd")(C.byref(d), _p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta),
                                          _p(dx), _p(dg), _p(db), training, _p(ws), ws.numel(), self._stream()),
                  "norm_act_bwd")
        return dx, dg, db

    def norm_act_bwd_pool(self, x, dskip, dpool, mean, rstd, gamma, beta, groups, act, training=1, eps=1e-5, slope=0.01):
        """norm backward whose incoming gradient is dskip (may be None) + the un-pooled dpool -> (dx, dgamma, dbeta);
        dense tensors -- HIP library only"""
        x, dskip, dpool, mean, rstd, gamma, beta = map(self.to, (x, dskip, dpool, mean, rstd, gamma, beta))
        N, Cc, D, H, W = x.shape
        d = self.norm_desc(x, groups, act, eps, slope)
        dx, dg, db = self.empty(*x.shape), self.empty(Cc), self.empty(Cc)
        ws = self._ws("norm_workspace", d)
        self._chk(self.fn("norm_act_bwd_pool")(C.byref(d), _p(x), _p(dskip), 0, _p(dpool), 0, D, H, W, _p(mean), _p(rstd),
                                               _p(gamma), _p(beta), _p(dx), _p(dg), _p(db), training, _p(ws), ws.numel(),
                                               self._stream()), "norm_act_bwd_pool")
        return dx, dg, db

    def norm_act_pool_fwd(self, x, mean, rstd, gamma, beta, groups, act, eps=1e-5, slope=0.01, out=None, out_pooled=None):
        """norm + activation with AvgPool3d(2, 2) of the result as second output -> (y, pooled)"""
        x, mean, rstd, gamma, beta = map(self.to, (x, mean, rstd, gamma, beta))
        N, Cc, D, H, W = x.shape
        y, pooled = self._out(out, x.shape), self._out(out_pooled, (N, Cc, D // 2, H // 2, W // 2))
        d = self.norm_desc(x, groups, act, eps, slope, _bs(x), _bs(y))
        self._chk(self.fn("norm_act_pool_fwd")(C.byref(d), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(y), _p(pooled),
                                               _bs(pooled), D, H, W, self._stream()), "norm_act_pool_fwd")
        return y, pooled

    def norm_act_bwd_h16(self, x, dy, mean, rstd, gamma, beta, groups, act, compute, training=1, eps=1e-5, slope=0.01,
                         out=None, out16=None):
        """norm backward that also emits dx as c8 -> (dx, dgamma, dbeta, dx16 [N, CB, S, 8])"""
        x, dy, mean, rstd, gamma, beta = map(self.to, (x, dy, mean, rstd, gamma, beta))
        N, Cc = x.shape[:2]
        S = x.numel() // (N * Cc)
        dx = self._out(out, x.shape)
        assert _bs(dx) == _bs(x) or N == 1
        d = self.norm_desc(x, groups, act, eps, slope, _bs(x), _bs(dy))
        dg = self.empty(Cc) if gamma is not None else None
        db = self.empty(Cc) if gamma is not None else None
        dx16 = self._out(out16, (N, (Cc + 7) // 8, S, 8), self.dt16(compute))
        ws = self._ws("norm_workspace", d)
        self._chk(self.fn("norm_act_bwd_h16")(C.byref(d), _p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dx),
                                              _p(dg), _p(db), training, _p(dx16), _bs(dx16), compute, _p(ws), ws.numel(),
                                              self._stream()), "norm_act_bwd_h16")
        return dx, dg, db, dx16

    # ---- synchronised batch norm: the local halves around the all-reduce (total_count None = this rank's own count)
    def norm_sums(self, x=None, stat_partials=None, x_shape=None, eps=1e-5):
        """-> sums [2 C + 1] (double): per channel (sum, sum of squares), then the element count.  From x (tensor or Slot), or
        from a conv's epilogue partials [N, P, C, 2] of a tensor of shape x_shape"""
        x, stat_partials = self.to(x), self.to(stat_partials)
        N, Cc = (x.shape if x is not None else x_shape)[:2]
        S = (x.numel() if x is not None else torch.Size(x_shape).numel()) // (N * Cc)
        d = NormDesc(N, Cc, S, 0, 0, eps, 0.01, _bs(x) if x is not None else 0, 0, 0)
        sums = self.empty(2 * Cc + 1, dtype=torch.float64)
        ws = self._ws("norm_workspace", d)
        slots = stat_partials.shape[1] if stat_partials is not None else 0
        self._chk(self.fn("norm_sums")(C.byref(d), _p(x), _p(stat_partials), slots, _p(sums), _p(ws), ws.numel(), self._stream()),
                  "norm_sums")
        return sums

    def norm_stats_from_sums(self, sums, x_shape, eps=1e-5, running=None, momentum=0.1):
        N, Cc = x_shape[:2]
        d = NormDesc(N, Cc, torch.Size(x_shape).numel() // (N * Cc), 0, 0, eps, 0.01, 0, 0, 0)
        mean, rstd = self.empty(Cc), self.empty(Cc)
        rm = rv = None
        if running is not None:
            rm, rv = self.to(running[0]).clone(), self.to(running[1]).clone()
        self._chk(self.fn("norm_stats_from_sums")(C.byref(d), _p(sums), _p(mean), _p(rstd), _p(rm), _p(rv), momentum,
                                                  self._stream()), "norm_stats_from_sums")
        return mean, rstd, rm, rv

    def norm_act_bwd_reduce(self, x, dy, mean, rstd, gamma, beta, groups, act, training=1, total_count=None, eps=1e-5,
                            slope=0.01):
        """first half of norm_act_bwd -> (stat_m [num_stats, 2], dgamma, dbeta); total_count: device double, or None"""
        x, dy, mean, rstd, gamma, beta = map(self.to, (x, dy, mean, rstd, gamma, beta))
        d = self.norm_desc(x, groups, act, eps, slope, _bs(x), _bs(dy))
        stat_m = self.empty(self.fn("norm_num_stats")(C.byref(d)), 2)
        dg = self.empty(x.shape[1]) if gamma is not None else None
        db = self.empty(x.shape[1]) if gamma is not None else None
        ws = self._ws("norm_workspace", d)
        self._chk(self.fn("norm_act_bwd_reduce")(C.byref(d), _p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dg),
                                                 _p(db), training, _p(total_count), _p(stat_m), _p(ws), ws.numel(),
                                                 self._stream()), "norm_act_bwd_reduce")
        return stat_m, dg, db

    def norm_act_bwd_apply(self, x, dy, mean, rstd, gamma, beta, stat_m, groups, act, compute=None, eps=1e-5, slope=0.01,
                           out=None, out16=None):
        """second half -> (dx, dx16); compute 1 / 2: also the c8 twin of dx (None: dx16 is None)"""
        x, dy, mean, rstd, gamma, beta = map(self.to, (x, dy, mean, rstd, gamma, beta))
        N, Cc = x.shape[:2]
        dx = self._out(out, x.shape)
        assert _bs(dx) == _bs(x) or N == 1
        d = self.norm_desc(x, groups, act, eps, slope, _bs(x), _bs(dy))
        dx16 = self._out(out16, (N, (Cc + 7) // 8, x.numel() // (N * Cc), 8), self.dt16(compute)) if compute else None
        self._chk(self.fn("norm_act_bwd_apply")(C.byref(d), _p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(stat_m),
                                                _p(dx), _p(dx16), _bs(dx16), compute or 0, self._stream()),
                  "norm_act_bwd_apply")
        return dx, dx16

    def norm_act_bwd_c8_reduce(self, x16, dy16, dpool16, Cc, spatial, mean, rstd, gamma, beta, groups, act, compute, training=1,
                               total_count=None, unscale=1.0, eps=1e-5, slope=0.01):
        """first half of norm_act_bwd_c8 -> (stat_m, dgamma, dbeta)"""
        mean, rstd, gamma, beta = map(self.to, (mean, rstd, gamma, beta))
        D, H, W = spatial
        d = NormDesc(x16.shape[0], Cc, x16.shape[2], groups, act, eps, slope, 0, 0, 0)
        stat_m = self.empty(self.fn("norm_num_stats")(C.byref(d)), 2)
        dg = self.empty(Cc) if gamma is not None else None
        db = self.empty(Cc) if gamma is not None else None
        ws = self._ws("norm_workspace", d)
        self._chk(self.fn("norm_act_bwd_c8_reduce")(C.byref(d), _p(x16), _bs(x16), _p(dy16), _bs(dy16), _p(dpool16), _bs(dpool16),
                                                    D, H, W, _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dg), _p(db), training,
                                                    _p(total_count), float(unscale), _p(stat_m), compute, _p(ws), ws.numel(),
                                                    self._stream()), "norm_act_bwd_c8_reduce")
        return stat_m, dg, db

    def norm_act_bwd_c8_apply(self, x16, dy16, dpool16, Cc, spatial, mean, rstd, gamma, beta, stat_m, groups, act, compute,
                              eps=1e-5, slope=0.01, out=None):
        """second half -> dx16"""
        mean, rstd, gamma, beta = map(self.to, (mean, rstd, gamma, beta))
        D, H, W = spatial
        d = NormDesc(x16.shape[0], Cc, x16.shape[2], groups, act, eps, slope, 0, 0, 0)
        dx16 = self._out(out, x16.shape, x16.dtype, fill=7.0)
        self._chk(self.fn("norm_act_bwd_c8_apply")(C.byref(d), _p(x16), _bs(x16), _p(dy16), _bs(dy16), _p(dpool16),
                                                   _bs(dpool16), D, H, W, _p(mean), _p(rstd), _p(gamma), _p(beta), _p(stat_m),
                                                   _p(dx16), _bs(dx16), compute, self._stream()), "norm_act_bwd_c8_apply")
        return dx16

    # -------------------------------------------------- pool / upsample / softmax
    # (every tensor argument may be a Slot, `out` an output Slot: pointers and batch strides then come from the slots)
    def avgpool_fwd(self, x, out=None):
        x = self.to(x)
        N, Cc, D, H, W = x.shape
        y = self._out(out, (N, Cc, D // 2, H // 2, W // 2))
        self._chk(self.fn("avgpool3d_2x_fwd")(_p(x), _p(y), N, Cc, D, H, W, _bs(x), _bs(y), self._stream()), "avgpool_fwd")
        return y

    def avgpool_bwd(self, dy, x_shape, out=None):
        dy = self.to(dy)
        N, Cc, D, H, W = x_shape
        dx = self._out(out, x_shape)
        self._chk(self.fn("avgpool3d_2x_bwd")(_p(dy), _p(dx), N, Cc, D, H, W, _bs(dy), _bs(dx), self._stream()), "avgpool_bwd")
        return dx

    def avgpool_bwd_add(self, dy, add, x_shape, out=None):
        dy, add = self.to(dy), self.to(add)
        N, Cc, D, H, W = x_shape
        dx = self._out(out, x_shape)
        self._chk(self.fn("avgpool3d_2x_bwd_add")(_p(dy), _p(add), _p(dx), N, Cc, D, H, W, _bs(dy), _bs(add), _bs(dx),
                                                  self._stream()), "avgpool_bwd_add")
        return dx

    def maxpool_fwd(self, x, route=True, out=None):
        """-> (y, route bytes [N, C, D/2, H/2, W/2] uint8 or None)"""
        x = self.to(x)
        N, Cc, D, H, W = x.shape
        oshape = (N, Cc, D // 2, H // 2, W // 2)
        y = self._out(out, oshape)
        idx = self._out(None, oshape, torch.uint8, fill=255) if route else None
        self._chk(self.fn("maxpool3d_2x_fwd")(_p(x), _p(y), _p(idx), N, Cc, D, H, W, _bs(x), _bs(y), self._stream()), "maxpool_fwd")
        return y, idx

    def maxpool_bwd(self, dy, idx, add, x_shape, out=None):
        dy, add = self.to(dy), self.to(add)
        N, Cc, D, H, W = x_shape
        dx = self._out(out, x_shape)
        self._chk(self.fn("maxpool3d_2x_bwd")(_p(dy), _p(idx), _p(add), _p(dx), N, Cc, D, H, W, _bs(dy), _bs(add), _bs(dx),
                                              self._stream()), "maxpool_bwd")
        return dx

    def maxpool_fwd_h16(self, x16, Cc, spatial, compute, route=True, out=None):
        """-> (y16, route bytes [N, CB, S/8, 8] uint8 or None)"""
        D, H, W = spatial
        N, CB = x16.shape[0], (Cc + 7) // 8
        y16 = self._out(out, (N, CB, D * H * W // 8, 8), x16.dtype, fill=7.0)
        idx8 = self._out(None, (N, CB, D * H * W // 8, 8), torch.uint8, fill=255) if route else None
        self._chk(self.fn("maxpool3d_2x_fwd_h16")(_p(x16), _p(y16), _p(idx8), N, Cc, D, H, W, _bs(x16), _bs(y16), compute,
                                                  self._stream()), "maxpool_fwd_h16")
        return y16, idx8

    def maxpool_bwd_h16(self, dpool16, idx8, dskip16, Cc, spatial, compute, out=None):
        D, H, W = spatial
        N = dpool16.shape[0]
        dx16 = self._out(out, (N, (Cc + 7) // 8, D * H * W, 8), dpool16.dtype, fill=7.0)
        self._chk(self.fn("maxpool3d_2x_bwd_h16")(_p(dpool16), _p(idx8), _p(dskip16), _p(dx16), N, Cc, D, H, W, _bs(dpool16),
                                                  _bs(dskip16), _bs(dx16), compute, self._stream()), "maxpool_bwd_h16")
        return dx16

    def upsample_fwd(self, x, out=None):
        x = self.to(x)
        N, Cc, D, H, W = x.shape
        y = self._out(out, (N, Cc, 2 * D, 2 * H, 2 * W))
        self._chk(self.fn("upsample_trilinear2x_fwd")(_p(x), _p(y), N, Cc, D, H, W, _bs(x), _bs(y), self._stream()),
                  "upsample_fwd")
        return y

    def upsample_bwd(self, dy, x_shape, out=None):
        dy = self.to(dy)
        N, Cc, D, H, W = x_shape
        dx = self._out(out, x_shape)
        self._chk(self.fn("upsample_trilinear2x_bwd")(_p(dy), _p(dx), N, Cc, D, H, W, _bs(dy), _bs(dx), self._stream()),
                  "upsample_bwd")
        return dx

    def space_to_depth(self, x, out=None):
        x = self.to(x)
        N, Cc, D, H, W = x.shape
        y = self._out(out, (N, Cc * 8, D // 2, H // 2, W // 2))
        self._chk(self.fn("space_to_depth2")(_p(x), _p(y), N, Cc, D, H, W, _bs(x), _bs(y), self._stream()), "space_to_depth2")
        return y

    def depth_to_space(self, x, out=None):
        x = self.to(x)
        N, C8, D, H, W = x.shape
        y = self._out(out, (N, C8 // 8, 2 * D, 2 * H, 2 * W))
        self._chk(self.fn("depth_to_space2")(_p(x), _p(y), N, C8 // 8, 2 * D, 2 * H, 2 * W, _bs(x), _bs(y), self._stream()),
                  "depth_to_space2")
        return y

    def copy_channels(self, x, out=None):
        x = self.to(x)
        N, Cc = x.shape[:2]
        S = x.numel() // (N * Cc)
        y = self._out(out, x.shape)
        self._chk(self.fn("copy_channels")(_p(x), _p(y), N, Cc, S, _bs(x), _bs(y), self._stream()), "copy_channels")
        return y

    def dwi_mean(self, x, idx, out=None):
        """x: [1, channels, D, H, W] (tensor or Slot) -> [1, 1, D, H, W] mean over the channels `idx`, summed in that
        order (m355_dwi_mean has no stride arguments: only the pointers move) -- HIP library only"""
        x = self.to(x)
        _, Cc, D, H, W = x.shape
        y = self._out(out, (1, 1, D, H, W))
        it = torch.tensor(list(idx), dtype=torch.int32, device=self.device)
        self._chk(self.fn("dwi_mean")(_p(x), Cc, self._i3((D, H, W)), _p(it), len(idx), _p(y), self._stream()), "dwi_mean")
        return y

    def blur_weight_fwd(self, w, scale, standardize, transposed):
        w, scale = self.to(w), self.to(scale)
        A, B = w.shape[:2]
        wexp = self.empty(8 * B, A, 3, 3, 3) if transposed else self.empty(A, 8 * B, 3, 3, 3)
        ms = self.empty(A, 2)
        self._chk(self.fn("blur_weight_fwd")(_p(w), _p(scale), _p(wexp), _p(ms), A, B, int(standardize),
                                             int(transposed), self._stream()), "blur_weight_fwd")
        return wexp, ms

    def blur_weight_bwd(self, dwexp, w, scale, ms, standardize, transposed):
        dwexp, w, scale, ms = map(self.to, (dwexp, w, scale, ms))
        A, B = w.shape[:2]
        dw = self.empty(*w.shape, dtype=w.dtype)
        self._chk(self.fn("blur_weight_bwd")(_p(dwexp), _p(w), _p(scale), _p(ms), _p(dw), A, B, int(standardize),
                                             int(transposed), self._stream()), "blur_weight_bwd")
        return dw

    def weight_standardize_fwd(self, w):
        w = self.to(w)
        A, n = w.shape[0], w[0].numel()
        wn, ms = self.empty(*w.shape, dtype=w.dtype), self.empty(A, 2)
        self._chk(self.fn("weight_standardize_fwd")(_p(w), _p(wn), _p(ms), A, n, self._stream()), "weight_standardize_fwd")
        return wn, ms

    def weight_standardize_bwd(self, dwn, w, ms):
        dwn, w, ms = map(self.to, (dwn, w, ms))
        dw = self.empty(*w.shape, dtype=w.dtype)
        self._chk(self.fn("weight_standardize_bwd")(_p(dwn), _p(w), _p(ms), _p(dw), w.shape[0], w[0].numel(),
                                                    self._stream()), "weight_standardize_bwd")
        return dw

    def patch_gather_padded(self, vol, loc, ps, border, mode, value=0.0):
        vol, loc = self.to(vol), self.to(loc.to(torch.int32))
        Cc, V0, V1, V2 = vol.shape
        P = loc.shape[0]
        out = self.empty(P, Cc, *ps)
        self._chk(self.fn("patch_gather_padded")(_p(vol), _p(loc), _p(out), P, Cc, V0, V1, V2, ps[0], ps[1], ps[2],
                                                 border[0], border[1], border[2], mode, float(value), self._stream()),
                  "patch_gather_padded")
        return out

    def patch_aggregate_grid(self, tiles, axes, vshape, border=(0, 0, 0)):
        tiles = self.to(tiles)
        P, Cc, ps0, ps1, ps2 = tiles.shape
        starts = torch.tensor([v for a in axes for v in a], dtype=torch.int32, device=self.device)
        out = self.empty(Cc, *vshape)
        self._chk(self.fn("patch_aggregate_grid")(_p(tiles), _p(starts), len(axes[0]), len(axes[1]), len(axes[2]), _p(out), Cc,
                                                  *vshape, ps0, ps1, ps2, *border, self._stream()), "patch_aggregate_grid")
        return out

    def patch_finalize_crop(self, accum, count, border):
        accum, count = self.to(accum), self.to(count)
        Cc, P0, P1, P2 = accum.shape
        out = self.empty(Cc, P0 - 2 * border[0], P1 - 2 * border[1], P2 - 2 * border[2])
        self._chk(self.fn("patch_finalize_crop")(_p(accum), _p(count), _p(out), Cc, P0, P1, P2, border[0], border[1],
                                                 border[2], self._stream()), "patch_finalize_crop")
        return out

    # ---------------------------------------------------------------- ensembles
    @staticmethod
    def _i3(v):
        return (C.c_int32 * 3)(*[int(a) for a in v])

    def flip_permute(self, x, perm, flip_mask):
        x = self.to(x)
        N, Cc = x.shape[:2]
        sp = x.shape[2:]
        y = self.empty(N, Cc, *[sp[p] for p in perm])
        self._chk(self.fn("flip_permute")(_p(x), _p(y), N, Cc, self._i3(sp), self._i3(perm), flip_mask, self._stream()),
                  "flip_permute")
        return y

    def ensemble(self, preds, transforms, canonical_spatial, strategy):
        """preds[e]: member prediction in member orientation; transforms[e] = (perm, flip_mask) -> (result, votes)"""
        mode = 0 if strategy == "mean" else 1
        N, Cc = preds[0].shape[:2]
        shape = (N, Cc) + tuple(canonical_spatial)
        acc = self.empty(*shape) if mode == 0 else self.empty(*shape, dtype=torch.int32)
        for e, (p, (perm, fm)) in enumerate(zip(preds, transforms)):
            p = self.to(p)
            self._chk(self.fn("ensemble_accumulate")(_p(p), _p(acc) if mode == 0 else None, _p(acc) if mode == 1 else None,
                                                     N, Cc, self._i3(canonical_spatial), self._i3(perm), fm, mode,
                                                     1 if e == 0 else 0, self._stream()), "ensemble_accumulate")
        S = shape[2] * shape[3] * shape[4]
        out = self.empty(*shape) if mode == 0 else self.empty(*shape, dtype=torch.int64)
        self._chk(self.fn("ensemble_finalize")(_p(acc) if mode == 0 else None, _p(acc) if mode == 1 else None,
                                               _p(out) if mode == 0 else None, _p(out) if mode == 1 else None, N, Cc, S,
                                               len(preds), mode, self._stream()), "ensemble_finalize")
        return out, acc

    def softmax_fwd(self, x, inner=1, diag_bias=0.0):
        x = self.to(x)
        N, Ct = x.shape[:2]
        S = x.numel() // (N * Ct)
        y = self.empty(*x.shape, dtype=x.dtype)
        self._chk(self.fn("softmax_fwd")(_p(x), _p(y), N, Ct // inner, inner, S, diag_bias, self._stream()),
                  "softmax_fwd")
        return y

    def softmax_bwd(self, y, dy, inner=1):
        y, dy = self.to(y), self.to(dy)
        N, Ct = y.shape[:2]
        S = y.numel() // (N * Ct)
        dx = self.empty(*y.shape, dtype=y.dtype)
        self._chk(self.fn("softmax_bwd")(_p(y), _p(dy), _p(dx), N, Ct // inner, inner, S, self._stream()),
                  "softmax_bwd")
        return dx

    # ------------------------------------------------------------------ loss
    def loss_fwd(self, p, t, dice_weight=0.5, cw=None, square=True):
        p, t, cw = map(self.to, (p, t, cw))
        N, Cc = p.shape[:2]
        S = p.numel() // (N * Cc)
        out3, sums = self.empty(3), self.empty(N * Cc * 4)
        nws = self.lib.m355_hybrid_loss_workspace(N, Cc, S) if self.backend == "hip" else 16
        ws = self._workspace(nws)
        self._chk(self.fn("hybrid_loss_fwd")(_p(p), _p(t), N, Cc, S, dice_weight, _p(cw), int(square), _p(out3),
                                             _p(sums), _p(ws), ws.numel(), self._stream()), "loss_fwd")
        return out3, sums

    def loss_bwd(self, p, t, sums, dloss=1.0, dice_weight=0.5, cw=None, square=True):
        p, t, sums, cw = map(self.to, (p, t, sums, cw))
        N, Cc = p.shape[:2]
        S = p.numel() // (N * Cc)
        g = torch.tensor([dloss], dtype=torch.float32, device=self.device)
        dp = self.empty(*p.shape, dtype=p.dtype)
        self._chk(self.fn("hybrid_loss_bwd")(_p(p), _p(t), _p(sums), _p(g), N, Cc, S, dice_weight, _p(cw),
                                             int(square), _p(dp), self._stream()), "loss_bwd")
        return dp

    # ------------------------------------------------------ patches / evaluation
    def patch_gather(self, vol, loc, ps):
        vol, loc = self.to(vol), self.to(loc.to(torch.int32))
        Cc, V0, V1, V2 = vol.shape
        P = loc.shape[0]
        out = self.empty(P, Cc, *ps)
        self._chk(self.fn("patch_gather")(_p(vol), _p(loc), _p(out), P, Cc, V0, V1, V2, *ps, self._stream()),
                  "patch_gather")
        return out

    def patch_aggregate(self, patches, loc, vshape):
        patches, loc = self.to(patches), self.to(loc.to(torch.int32))
        P, Cc = patches.shape[:2]
        ps = patches.shape[2:]
        accum = torch.zeros((Cc,) + tuple(vshape), device=self.device)
        count = torch.zeros(tuple(vshape), device=self.device)
        self._chk(self.fn("patch_accumulate")(_p(patches), _p(loc), _p(accum), _p(count), P, Cc, *vshape, *ps,
                                              self._stream()), "patch_accumulate")
        out = self.empty(*accum.shape, dtype=accum.dtype)
        self._chk(self.fn("patch_finalize")(_p(accum), _p(count), _p(out), Cc, count.numel(), self._stream()),
                  "patch_finalize")
        return out, count

    def argmax_confusion(self, prob, target):
        prob, target = self.to(prob), self.to(target.to(torch.int32))
        N, Cc = prob.shape[:2]
        S = prob.numel() // (N * Cc)
        am = self.empty(*target.shape, dtype=torch.int32)
        counts = self.empty(N, Cc, 4, dtype=torch.int64)
        self._chk(self.fn("argmax_confusion")(_p(prob), _p(target), _p(am), _p(counts), N, Cc, S, self._stream()),
                  "argmax_confusion")
        return am, counts
