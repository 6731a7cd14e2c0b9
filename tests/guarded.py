"""A guarded buffer arena: where the kernels read and write, next to what they compute.

Every buffer is one uint8 tensor of  guard + payload + guard  bytes, all of it filled with 0xFF first -- a NaN in fp32 and in fp64,
and a fixed pattern to compare with.  The payload is then filled with 0xFF or 0x00, as the caller says, and handed out as a typed
view.  After an exec,
    check_guards  every guard byte of every buffer still is 0xFF (a store past either end of `in`, `out`, `back` or the work area);
    check_inputs  every registered input is bit-identical to its host copy;
and because the guards around an input are NaN, a load past its end that feeds a result turns that result into a NaN.  Running the
same plans once on 0xFF payloads and once on 0x00 payloads and comparing the results bit for bit shows a result that depends on what
`out`, `back` or the work area held before.

guard = max(2 MiB, the plan's dfft_domain_size()) rounded up to 2 MiB: wider than any tile, row or slice a kernel could be off by,
and the payload keeps the alignment of the allocation.  offset256=True puts 256 more bytes in front of the payload: the granularity
the library rounds its own slices to, and what a caller's view into a larger allocation looks like.

The runners of the GPU tests take an `arena=` keyword (None: they allocate exact-size tensors as before); tests/test_gpu_footprint.py
drives them, tests/test_cpu_guarded.py proves on CPU tensors that the arena sees what it is for.  Device-agnostic: device="cuda" in
the GPU tests, "cpu" in the self-test."""
import os

import numpy as np
import torch

MIB2 = 2 << 20
GUARD_BYTE = 0xFF


def guard_bytes(domain_bytes):
    return (max(MIB2, int(domain_bytes)) + MIB2 - 1) // MIB2 * MIB2


class _Buffer:
    def __init__(self, name, whole, front, nbytes, view, host):
        self.name, self.whole, self.front, self.nbytes, self.view, self.host = name, whole, front, nbytes, view, host

    @property
    def payload(self):
        return self.whole[self.front:self.front + self.nbytes]


class Arena:
    def __init__(self, device, fill=GUARD_BYTE, offset256=False, domain_bytes=0):
        self.device, self.fill, self.offset256 = device, fill, offset256
        self.guard = guard_bytes(domain_bytes)
        self.buffers = []
        self._once = {}

    # -- allocation ---------------------------------------------------------------------
    def domain(self, domain_bytes):
        """the guards of the buffers made from now on cover a plan with that dfft_domain_size() (they never shrink)"""
        self.guard = max(self.guard, guard_bytes(domain_bytes))

    def _make(self, nbytes, dtype, fill, name, host=None):
        nbytes = int(nbytes)
        front = self.guard + (256 if self.offset256 else 0)
        whole = torch.full((front + nbytes + self.guard,), GUARD_BYTE, dtype=torch.uint8, device=self.device)
        payload = whole[front:front + nbytes]
        if host is not None:
            payload.copy_(torch.frombuffer(bytearray(host), dtype=torch.uint8))
        elif fill != GUARD_BYTE:
            payload.fill_(fill)
        b = _Buffer(f"{name or 'buffer'}#{len(self.buffers)}", whole, front, nbytes, payload.view(dtype), host)
        self.buffers.append(b)
        return b.view

    def buffer(self, nbytes, dtype, fill=None, name=None):
        """a typed view of nbytes of payload filled with byte `fill` (0xFF or 0x00; default: the arena's), guards on both sides"""
        fill = self.fill if fill is None else fill
        assert fill in (0x00, GUARD_BYTE), fill
        return self._make(nbytes, dtype, fill, name)

    def input(self, np_array, name=None):
        """a guarded buffer holding the array, as a tensor of its shape and type; the host copy is what check_inputs compares with"""
        a = np.ascontiguousarray(np_array)
        return self._make(a.nbytes, torch.from_numpy(a.reshape(-1)[:1].copy()).dtype, None, name or "in", host=a.tobytes()).reshape(a.shape)

    def plan_buffers(self, plan, block, out_dtype, rank=0):
        """the buffers of one rank of a plan initialised with allocate=False: `in` holding block, `out` of dfft_domain_size() bytes,
        `back` of the block's size, and a caller-owned work area of dfft_work_size_device() bytes, which the plan is given"""
        self.domain(plan.getDomainSize())
        d_in = self.input(block, f"in[{rank}]")
        d_out = self.buffer(plan.getDomainSize(), out_dtype, name=f"out[{rank}]")
        d_back = self.buffer(block.nbytes, d_in.dtype, name=f"back[{rank}]").reshape(block.shape)
        self.work_area(plan, rank)
        return d_in, d_out, d_back

    def work_area(self, plan, rank=0):
        self.domain(plan.getDomainSize())
        work = self.buffer(plan.getWorkSizeDevice(), torch.uint8, name=f"work[{rank}]")
        plan.setWorkArea(work)
        assert plan.getWorkAreaDevice() == work.data_ptr(), "the plan does not run on the caller's work area"
        _record(f"rank {rank}: guard {self.guard} B{' + 256' if self.offset256 else ''}, domain {plan.getDomainSize()} B, work area {plan.getWorkSizeDevice()} B")
        return work

    def once(self, key, make):
        """make() at the first call, its result again at every later one: the second run of a case (the other payload fill) uses the
        plans and buffers of the first"""
        if key not in self._once:
            self._once[key] = make()
        return self._once[key]

    def refill(self, keep=()):
        """every buffer that is not an input gets the arena's payload fill again, except the tensors in `keep`"""
        kept = {t.data_ptr() for t in keep}
        for b in self.buffers:
            if b.host is None and b.view.data_ptr() not in kept:
                b.payload.fill_(self.fill)
        self.sync()

    def sync(self):
        if str(self.device).startswith("cuda"):
            torch.cuda.synchronize()

    # -- checks -------------------------------------------------------------------------
    def check_guards(self, what):
        """every guard byte of every buffer still is 0xFF; the report gives offsets relative to the payload (negative: in front of
        it; from the payload's size on: behind it)"""
        self.sync()
        sides = [(b, side, g) for b in self.buffers for side, g in (("front", b.whole[:b.front]), ("back", b.whole[b.front + b.nbytes:]))]
        if not bool(torch.stack([(g != GUARD_BYTE).any() for _, _, g in sides]).any()):
            return
        lines = []
        for b, side, g in sides:
            at = torch.nonzero(g != GUARD_BYTE).reshape(-1)
            if at.numel():
                base = -b.front if side == "front" else b.nbytes
                lines.append(f"{b.name} ({b.nbytes} bytes), {side} guard: {at.numel()} bytes changed, offsets {base + int(at[0])} .. {base + int(at[-1])} "
                             f"relative to the payload")
        raise AssertionError(f"{what}: written outside a buffer -- " + "; ".join(lines))

    def check_inputs(self, what):
        """every registered input is bit-identical to its host copy"""
        self.sync()
        for b in self.buffers:
            if b.host is None:
                continue
            now = b.payload.cpu().numpy()
            if now.tobytes() != b.host:
                at = np.nonzero(now != np.frombuffer(b.host, dtype=np.uint8))[0]
                raise AssertionError(f"{what}: input {b.name} was modified -- {at.size} bytes differ, offsets {int(at[0])} .. {int(at[-1])}")


def assert_written(block, what):
    """no entry of a result still is the NaN its buffer was filled with (or became one through a load outside an input)"""
    block = np.asarray(block)
    bad = np.isnan(block)
    if bad.any():
        k = np.unravel_index(int(np.argmax(bad)), block.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {block.size} entries are NaN, the first at {tuple(int(i) for i in k)}: "
                             f"never written, or computed from a read outside an input")


def _record(line):
    """DFFT_FOOTPRINT_TABLE=<file>: the guard and work-area sizes of every case, under the id of the running test"""
    path = os.environ.get("DFFT_FOOTPRINT_TABLE")
    if path:
        with open(path, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0].split('::')[-1]}: {line}\n")
