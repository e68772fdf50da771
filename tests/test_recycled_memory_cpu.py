"""Self-test of the recycled-memory harness of raw_ops.py (RawOps.scratch, Scratch, PoisonedEmpty, assert_recycled) on the
oracle backend and CPU tensors: the fills hold the stated bits, "stale" hands the same storage out again, the tail guard
and the comparison catch the bugs they are there for, and everything is undone on exit -- so a green GPU run of
test_recycled_memory_gpu.py means the kernels were really handed dirty memory."""
import pytest
import torch

import raw_ops
from raw_ops import PoisonedEmpty, Slot, assert_recycled, bit_equal

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool]
NAN_BYTES = {   # little-endian bytes of one element of the "nan" fill
    torch.float32: (0x7FC0BEEF).to_bytes(4, "little"), torch.bfloat16: (0x7FC5).to_bytes(2, "little"),
    torch.float16: (0x7E55).to_bytes(2, "little"), torch.float64: (0x7FF80000C0DEBEEF).to_bytes(8, "little"),
    torch.int32: b"\x7f" * 4, torch.int64: b"\x7f" * 8, torch.uint8: b"\x7f", torch.bool: b"\x01"}


def raw(t):
    return bytes(t.contiguous().view(torch.uint8).flatten().tolist())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_each_mode_holds_the_stated_bits(oracle, dtype):
    size = torch.empty(0, dtype=dtype).element_size()
    want = {"zeros": b"\x00" * size, "ones": b"\xff" * size, "nan": NAN_BYTES[dtype], "stale": b"\x5a" * size}
    for mode, one in want.items():
        with oracle.scratch(mode) as s:
            t = oracle.empty(3, 5, dtype=dtype)
            c8 = oracle._out(None, (2, 3), dtype, fill=7.0)     # (the pre-fill of a c8 output gives way to the mode)
        assert t.shape == (3, 5) and t.dtype == dtype and raw(t) == one * 15, mode
        assert raw(c8) == one * 6 and s.outputs == 2 and s.workspaces == 0
    assert Slot.CANARY[torch.float32][1] == 0x7FC0BEEF and torch.isnan(torch.tensor(0x7FC0BEEF, dtype=torch.int32).view(torch.float32))
    if dtype.is_floating_point:
        with oracle.scratch("nan"):
            assert torch.isnan(oracle.empty(4, dtype=dtype)).all()


def test_default_mode_tracks_nothing(oracle):
    with oracle.scratch(None) as s:
        assert oracle._scratch is None
        ws, t = oracle._workspace(40), oracle._out(None, (2, 2), torch.float32, fill=7.0)
    assert ws.numel() == 40 and ws.untyped_storage().nbytes() == 40 and (t == 7.0).all()
    assert (s.workspaces, s.outputs, s.declared) == (0, 0, 0)


def test_workspace_fill_declared_size_and_tail(oracle):
    word = {"zeros": b"\x00" * 4, "ones": b"\xff" * 4, "nan": NAN_BYTES[torch.float32], "stale": b"\x5a" * 4}
    for mode, one in word.items():
        with oracle.scratch(mode) as s:
            ws = oracle._workspace(40)
            small = oracle._workspace(0)        # (a query of 0 still hands 16 bytes over, and counts 0 declared bytes)
            odd = oracle._workspace(19)
        assert ws.numel() == 40 and raw(ws) == one * 10 and small.numel() == 16
        assert raw(odd) == ({"nan": b"\x7f"}.get(mode, one[:1])) * 19
        assert (s.workspaces, s.declared) == (3, 59)
        whole = torch.empty(0, dtype=torch.uint8).set_(ws.untyped_storage())
        assert whole.numel() == 40 + raw_ops.TAIL_BYTES and raw(whole[40:]) == bytes([raw_ops.TAIL_CANARY]) * raw_ops.TAIL_BYTES


def test_stale_returns_the_identical_storage(oracle):
    def calls():
        a, b = oracle.empty(7), oracle.empty(7)       # one site, one size, two allocations: two buffers
        return a, b, oracle._workspace(64), oracle.empty(8)
    with oracle.scratch("stale") as s:
        first = calls()
        first[0].fill_(3.0)
        first[2].fill_(9)
        s.rewind()
        second = calls()
        assert [t.data_ptr() for t in first] == [t.data_ptr() for t in second]
        assert first[0].data_ptr() != first[1].data_ptr()
        assert (second[0] == 3.0).all() and (second[2] == 9).all(), "not refilled"
        third = calls()                                # no rewind: further allocations of the same sites
        assert not {t.data_ptr() for t in third} & {t.data_ptr() for t in first}
    with oracle.scratch("stale"):
        assert raw(oracle.empty(7)) == b"\x5a" * 28, "a new context starts from scratch"


def test_tail_guard_catches_one_byte_past_the_declared_size(oracle):
    def fake_op(over):
        ws = oracle._workspace(48)
        whole = torch.empty(0, dtype=torch.uint8).set_(ws.untyped_storage())
        whole[:48 + over] = 1
    for mode in ("zeros", "stale", "ones", "nan"):
        with oracle.scratch(mode):
            fake_op(0)
        with pytest.raises(AssertionError, match="past the declared 48"):
            with oracle.scratch(mode):
                fake_op(1)
        assert oracle._scratch is None


# ---- fake ops with the bugs the protocol is there for: y = 2 x + (sum of x, staged in workspace word 1)
SKIPS, READS = "skips output element 3", "reads workspace word 1 before writing it"


def _fake(oracle, x, bug):
    ws = oracle._workspace(16).view(torch.float32)
    y = oracle.empty(*x.shape)
    if bug != READS:
        ws[1] = 0.0
    ws[1] += x.sum()
    val = 2 * x + ws[1]
    keep = torch.arange(x.numel()) != (3 if bug == SKIPS else -1)
    y[keep] = val[keep]
    return {"y": y}


def _protocol(oracle, bug, modes=raw_ops.SCRATCH_MODES[1:]):
    x1, x2 = torch.arange(6.0), torch.arange(6.0) * 3 + 1

    def reference(got):
        torch.testing.assert_close(got["y"], 2 * x1 + x1.sum(), rtol=0, atol=0)
    assert_recycled(oracle, lambda: _fake(oracle, x1, bug), lambda: _fake(oracle, x2, bug), reference, modes=modes)


@pytest.mark.parametrize("mode", ["stale", "ones", "nan"])
@pytest.mark.parametrize("bug", [SKIPS, READS])
def test_protocol_fails_a_buggy_op_in_every_poisoning_mode(oracle, bug, mode):
    """both bugs pass on zeroed memory (the two clean runs agree, and the read-before-write even meets its reference)"""
    with pytest.raises(AssertionError, match=rf"\(b\) on '{mode}' scratch \['y'\] differ"):
        _protocol(oracle, bug, modes=(mode,))
    assert oracle._scratch is None
    with oracle.scratch("zeros"):
        y = _fake(oracle, torch.arange(6.0), READS)["y"]
    assert torch.equal(y, 2 * torch.arange(6.0) + 15.0)


def test_everything_is_restored_also_after_an_exception(oracle, monkeypatch):
    originals = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with pytest.raises(ZeroDivisionError):
        with oracle.scratch("nan"):
            1 / 0
    assert oracle._scratch is None
    with pytest.raises(ZeroDivisionError):
        with PoisonedEmpty(monkeypatch, "nan", device_type="cpu"):
            assert torch.empty is not originals[0]
            1 / 0
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == originals


def test_package_level_poisoning_fills_counts_and_leaves_other_devices_alone(monkeypatch):
    with PoisonedEmpty(monkeypatch, "nan", device_type="cpu") as p:
        got = [torch.empty(3), torch.empty_like(torch.zeros(2, 2)), torch.empty_strided((2, 3), (4, 1)),
               torch.zeros(2, dtype=torch.float64).new_empty(5), torch.empty((2,), dtype=torch.int64), torch.empty(0)]
        kept = torch.zeros(4)
    assert p.dirtied == 6 and all(torch.isnan(t).all() for t in got[:4]) and (kept == 0).all()
    assert raw(got[4]) == b"\x7f" * 16 and raw(got[3])[:8] == NAN_BYTES[torch.float64]
    for mode, byte in (("zeros", b"\x00"), ("ones", b"\xff")):
        with PoisonedEmpty(monkeypatch, mode, device_type="cpu"):
            assert raw(torch.empty(5, dtype=torch.float16)) == byte * 10
    with PoisonedEmpty(monkeypatch, "ones") as p:       # the default: CUDA results only
        torch.empty(3)
    assert p.dirtied == 0
    with pytest.raises(AssertionError):
        PoisonedEmpty(monkeypatch, "stale")
    # an element size without a fill is never counted as dirtied: refused by the raw harness, left alone at package level
    with pytest.raises(TypeError):
        raw_ops.dirty(torch.zeros(2, dtype=torch.complex128), "nan")
    with PoisonedEmpty(monkeypatch, "nan", device_type="cpu") as p:
        torch.empty(2, dtype=torch.complex128)
    assert p.dirtied == 0


def test_protocol_passes_a_correct_op_and_counts(oracle):
    _protocol(oracle, None)
    with pytest.raises(AssertionError, match=r"\(d\)"):
        assert_recycled(oracle, lambda: {"y": torch.zeros(2)}, lambda: None, lambda got: None)
    with pytest.raises(AssertionError, match=r"\(d\)"):
        assert_recycled(oracle, lambda: {"y": torch.zeros(2)}, lambda: None, lambda got: None, has_workspace=False)
    assert_recycled(oracle, lambda: {"y": oracle.empty(2).zero_()}, lambda: None, lambda got: None, has_workspace=False)
    assert oracle._scratch is None


def test_bit_equal_sees_nan_payloads_signed_zeros_and_masks():
    a = torch.tensor([0.0, float("nan"), 1.0])
    b = a.clone()
    assert bit_equal(a, b) and not torch.equal(a, b)
    b[0] = -0.0
    assert not bit_equal(a, b) and bit_equal(a, b, torch.tensor([False, True, True]))
    assert not bit_equal(a, a.double()) and bit_equal(None, None) and not bit_equal(a, None)
