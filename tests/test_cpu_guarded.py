"""The guarded arena of tests/guarded.py sees what it is for -- shown with torch ops on CPU tensors, no GPU and no kernel involved:
a byte written next to the payload or at the far end of a guard, one flipped bit of an input, an output entry that nobody wrote,
and the placement of the offset256 form.  This is the mutation evidence for tests/test_gpu_footprint.py: the harness is mutated,
never a kernel or a size formula."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import guarded  # noqa: E402


def fresh(offset256=False, fill=0xFF):
    arena = guarded.Arena("cpu", fill=fill, offset256=offset256)
    x = np.arange(24, dtype=np.float64).reshape(2, 3, 4) - 7.5
    d_in = arena.input(x)
    d_out = arena.buffer(40 * 16, torch.complex128, name="out")
    return arena, x, d_in, d_out


def whole_of(arena, view):
    b = next(b for b in arena.buffers if b.view.data_ptr() == view.data_ptr())
    return b, b.whole


def test_guard_size_and_layout():
    assert guarded.guard_bytes(0) == 2 << 20 and guarded.guard_bytes((2 << 20) + 1) == 4 << 20 and guarded.guard_bytes(6 << 20) == 6 << 20
    arena, x, d_in, d_out = fresh()
    arena.domain((2 << 20) + 256)
    big = arena.buffer(512, torch.float32, fill=0x00, name="later")
    for view, guard in ((d_in, 2 << 20), (d_out, 2 << 20), (big, 4 << 20)):
        b, whole = whole_of(arena, view)
        assert b.front == guard and whole.numel() == 2 * guard + b.nbytes and view.data_ptr() - whole.data_ptr() == guard
    assert d_in.dtype == torch.float64 and tuple(d_in.shape) == x.shape and np.array_equal(d_in.numpy(), x)
    assert d_out.dtype == torch.complex128 and d_out.numel() == 40 and bool(torch.isnan(d_out.real).all())      # 0xFF bytes: NaN
    assert bool(torch.isnan(arena.buffer(64, torch.float32)).all()) and bool(torch.isnan(arena.buffer(64, torch.float64)).all())
    assert bool((big == 0).all())
    arena.check_guards("untouched")
    arena.check_inputs("untouched")


@pytest.mark.parametrize("offset256", [False, True])
@pytest.mark.parametrize("where", ["1 before", "1 after", "far front", "far back"])
def test_one_byte_outside_the_payload_is_reported(where, offset256):
    arena, x, d_in, d_out = fresh(offset256)
    b, whole = whole_of(arena, d_out)
    at = {"1 before": b.front - 1, "1 after": b.front + b.nbytes, "far front": 0, "far back": whole.numel() - 1}[where]
    whole[at] = 0xFE      # one bit of one byte
    rel = at - b.front
    with pytest.raises(AssertionError) as e:
        arena.check_guards("probe")
    msg = str(e.value)
    assert msg.startswith("probe: ") and b.name in msg and ("front guard" if rel < 0 else "back guard") in msg
    assert f"1 bytes changed, offsets {rel} .. {rel} " in msg
    arena.check_inputs("probe")      # the inputs are not involved
    whole[at] = 0xFF
    arena.check_guards("restored")


def test_first_last_and_count_of_a_run_of_changed_bytes():
    arena, x, d_in, d_out = fresh()
    b, whole = whole_of(arena, d_in)
    whole[b.front + b.nbytes + 16:b.front + b.nbytes + 48:8] = 0      # 4 bytes behind the input
    with pytest.raises(AssertionError, match=rf"in#0 \({b.nbytes} bytes\), back guard: 4 bytes changed, offsets {b.nbytes + 16} \.\. {b.nbytes + 40} "):
        arena.check_guards("probe")


def test_a_store_into_the_payload_is_not_a_guard_failure():
    arena, x, d_in, d_out = fresh()
    d_out.fill_(1 + 2j)
    d_out[0], d_out[-1] = 3, 4
    arena.check_guards("payload written from end to end")


def test_one_flipped_bit_of_an_input_is_reported():
    arena, x, d_in, d_out = fresh()
    b, _ = whole_of(arena, d_in)
    b.payload[72] ^= 1      # the lowest mantissa bit of entry 9: the value changes by less than any tolerance would see
    assert np.allclose(d_in.numpy(), x, rtol=1e-13, atol=0) and not np.array_equal(d_in.numpy(), x)
    with pytest.raises(AssertionError, match=r"probe: input in#0 was modified -- 1 bytes differ, offsets 72 \.\. 72"):
        arena.check_inputs("probe")
    arena.check_guards("probe")
    b.payload[72] ^= 1
    arena.check_inputs("restored")


def test_an_entry_never_written_is_reported():
    arena, x, d_in, d_out = fresh()
    d_out.fill_(0)
    guarded.assert_written(d_out.numpy(), "all written")
    b, _ = whole_of(arena, d_out)
    b.payload[16 * 13 + 8:16 * 13 + 16] = 0xFF      # the imaginary part of entry 13 keeps the fill
    with pytest.raises(AssertionError, match=r"probe: 1 of 40 entries are NaN, the first at \(13,\)"):
        guarded.assert_written(d_out.numpy(), "probe")


def test_refill_restores_outputs_and_leaves_inputs_and_kept_buffers():
    arena, x, d_in, d_out = fresh(fill=0x00)
    back = arena.buffer(64, torch.float32, name="back")
    assert bool((d_out == 0).all()) and bool((back == 0).all())
    d_out.fill_(5)
    back.fill_(6)
    arena.refill(keep=[d_out])
    assert bool((d_out == 5).all()) and bool((back == 0).all()) and np.array_equal(d_in.numpy(), x)
    arena.fill = 0xFF
    arena.refill()
    assert bool(torch.isnan(d_out.real).all()) and bool(torch.isnan(back).all()) and np.array_equal(d_in.numpy(), x)
    arena.check_guards("refilled")
    arena.check_inputs("refilled")


def test_once_keeps_the_first_result():
    arena = guarded.Arena("cpu")
    made = []
    assert arena.once("k", lambda: made.append(1) or "first") == "first" and arena.once("k", lambda: made.append(1) or "second") == "first"
    assert made == [1] and arena.once("other", lambda: "third") == "third"


def test_offset256_placement():
    """256 bytes off the allocation's alignment: aligned to 256, not to 512"""
    arena, x, d_in, d_out = fresh(offset256=True)
    for view in (d_in, d_out):
        b, whole = whole_of(arena, view)
        off = view.data_ptr() - whole.data_ptr()
        assert off == b.front == (2 << 20) + 256 and off % 256 == 0 and off % 512 == 256
        assert whole.numel() == off + b.nbytes + (2 << 20)
    plain = fresh()[0]
    assert all((b.view.data_ptr() - b.whole.data_ptr()) % 512 == 0 for b in plain.buffers)
