"""CPU model of the product's pass descriptors (test infrastructure, not a product path).

The HIP kernels are addressed by `PassArgs` descriptors that the host builds per plan
(distributedfft_amd/csrc/pipeline.hip: build_pipeline, build_pipeline_zyx, build_pipeline_yzx,
build_pipeline_single).  This module reads those descriptors through the C ABI's introspection getters
(dfft_debug_get_pass / dfft_debug_get_point_table, host only) and executes the documented address
forms (fft_pass.hip.h: LoadKind / StoreKind, SegEntry) with numpy transforms, rank by rank, moving
blocks between virtual ranks with the plan's own chunked exchange tables.  It checks what a GPU run
cannot isolate: that every descriptor, segment table and per-point table of a plan describes a
consistent data flow that ends in the reference's output layout -- without a GPU.

The buffer routing is the library's own: the steps of the chain an exec would run
(dfft_debug_get_chain, which run_chain in dfft.hip executes), replayed step by step.
"""
import numpy as np

import distributedfft_amd as dfft

LINES, TILED, KMAJOR = 0, 1, 2
S_LINES, S_KMAJOR, S_SAME, S_TRANSPOSE = 0, 1, 2, 3
ESZ = {"double": 16, "float": 8}      # bytes per complex element; a real element is half of it
MODES = ["c2c", "c2c", "c2c", "r2c", "c2r", "r2c"]      # by line form of a chain step (dfft_chain_step::form)


def _seg(starts, lens, bases, n):
    """segment of point n (a number or an array of points): its start, length and base"""
    s = np.zeros(np.shape(n), dtype=np.int64)
    for q in range(1, len(starts)):
        s = np.where(np.asarray(n) >= starts[q], q, s)
    return np.asarray(starts, dtype=np.int64)[s], np.asarray(lens, dtype=np.int64)[s], np.asarray(bases, dtype=np.int64)[s]


class Pass:
    """one launch descriptor + its per-point tables"""

    def __init__(self, plan, name, index=0):
        self.esz = 16 if plan.precision == 1 else 8
        self.d = plan.debugPass(name, index)
        assert self.d is not None, (name, index)
        d = self.d
        self.TL = plan.getTileLines()
        self.l = ([int(v) for v in d.lstart[:d.lnseg]], [int(v) for v in d.llen[:d.lnseg]], [int(v) for v in d.lbase[:d.lnseg]])
        self.s = ([int(v) for v in d.sstart[:d.snseg]], [int(v) for v in d.slen[:d.snseg]], [int(v) for v in d.sbase[:d.snseg]])
        table = lambda store: np.array(plan.debugPointTable(name, index, store), dtype=np.int64).reshape(-1, 3).T      # noqa: E731
        self.ltab = table(False) if d.load_kind == TILED and d.lnseg >= 1 else None       # rows: base, ln, aux; one column per point
        self.stab = table(True) if d.store_kind in (S_SAME, S_TRANSPOSE) and d.snseg >= 1 else None

    def tile(self, line):
        b, l = np.divmod(line, self.TL)
        return b, l, np.minimum(self.TL, self.d.LB - b * self.TL)

    # load_offset / store_offset: element offset of point n (k) of line (a, line); `line` and n may be arrays that broadcast
    # (footprint: a column of lines against a row of points)

    def load_offset(self, a, line, n, NP):
        d, TL = self.d, self.TL
        b, l, tw = self.tile(line)
        if d.load_kind == LINES:
            return (a * d.AS_in + line * d.KS_in if d.KS_in else (a * d.LB + line) * NP) + n
        if d.load_kind == KMAJOR:
            return n * d.KS_in + a * d.AS_in + line
        s0, ln, bs = _seg(*self.l, n)
        if d.IA:                                   # one segment with explicit (padded) strides: closed form only
            assert d.lnseg == 1
            return bs + a * d.IA + b * d.IB + (n - s0) * tw + l
        off = bs + a * ln * d.LB + b * TL * ln + (n - s0) * tw + l
        base, tln, aux = self.ltab[:, n]            # the per-point table must say the same
        assert np.all(off == base + tln * (a * d.LB + b * TL) + aux * tw + l)
        return off

    def store_offset(self, a, line, k, NP):
        d, TL = self.d, self.TL
        b, l, tw = self.tile(line)
        if d.store_kind == S_LINES:
            return (a * d.AS_out + line * d.KS_out if d.KS_out else (a * d.LB + line) * NP) + k
        if d.store_kind == S_KMAJOR:
            return k * d.KS_out + a * d.AS_out + line
        s0, ln, bs = _seg(*self.s, k)
        base, tln, aux = self.stab[:, k]
        if d.store_kind == S_SAME:
            sk, sb = (d.SK or d.LB * d.LA), (d.SB or TL * d.LA)
            off = bs + (k - s0) * sk + b * sb + a * tw + l
            assert np.all(off == base + b * sb + a * tw + l)
            return off
        T2 = 1 << d.T2shift
        kt, kr = (k - s0) >> d.T2shift, (k - s0) & (T2 - 1)
        tw2 = np.minimum(T2, ln - kt * T2)
        off = bs + a * ln * d.LB + kt * T2 * d.LB + line * tw2 + kr
        assert np.all(off == base + tln * (a * d.LB) + line * aux)
        return off

    def sides(self, N, mode):
        """points per line and elements skipped by in_off / out_off (in elements of that side's type) on the load and the store side"""
        d = self.d
        nin = N // 2 + 1 if mode == "c2r" else N
        nout = N // 2 + 1 if mode == "r2c" else N
        return nin, nout, d.in_off // (self.esz // 2 if mode == "r2c" else self.esz), d.out_off // (self.esz // 2 if mode == "c2r" else self.esz)

    def run(self, src, dst, N, mode="c2c"):
        """mode: c2c (N complex points), r2c (N reals in -> N//2+1 out), c2r (N//2+1 in -> N reals out).
        src / dst are flat numpy arrays of the element type of that side."""
        d = self.d
        nin, nout, ioff, ooff = self.sides(N, mode)
        src = src[ioff:]
        dst = dst[ooff:]
        for a in range(d.na):
            for line in range(d.LB):
                x = src[self.load_offset(a, line, np.arange(nin), nin)]
                if mode == "r2c":
                    y = np.fft.rfft(x.real, N)
                elif mode == "c2r":
                    y = np.fft.irfft(x, N) * N
                else:
                    y = np.fft.ifft(x) * N if d.swap else np.fft.fft(x)
                dst[self.store_offset(a, line, np.arange(nout), nout)] = y[:nout]

    def footprint(self, N, mode="c2c"):
        """(loads, stores): what the launch reads from its source and writes to its destination buffer, as sorted arrays of indices in
        units of one REAL element from the start of the buffer (a complex element is two of them; real sides are half as wide).  The
        addresses are those of run(): load_offset / store_offset over every (a, line, point), per-point-table assertions included."""
        d = self.d
        nin, nout, ioff, ooff = self.sides(N, mode)
        wi, wo = (1 if mode == "r2c" else 2), (1 if mode == "c2r" else 2)
        cat = lambda v: np.concatenate(v + [np.zeros(0, dtype=np.int64)]).astype(np.int64)      # noqa: E731
        lines = np.arange(d.LB, dtype=np.int64)[:, None]
        ld = cat([np.ravel(self.load_offset(a, lines, np.arange(nin)[None, :], nin)) for a in range(d.na)])
        st = cat([np.ravel(self.store_offset(a, lines, np.arange(nout)[None, :], nout)) for a in range(d.na)])
        ld, st = (ld + ioff) * wi, (st + ooff) * wo
        assert len(np.unique(st)) == len(st), "a launch stores twice to one element"
        widen = lambda v, w: np.unique(v if w == 1 else np.concatenate([v, v + 1]))      # noqa: E731
        return widen(ld, wi), widen(st, wo)


class World:
    """P virtual ranks of one plan class on a small fp64 grid"""

    def __init__(self, cls, shape, P1, P2, c2c, chunks=None, precision="double", options=None):
        self.shape, self.P1, self.P2, self.c2c = shape, P1, P2, c2c
        self.esz = ESZ[precision]
        self.P = P1 * P2
        comm = dfft.Comm.local(self.P) if self.P > 1 else None
        self.plans = []
        for r in range(self.P):
            pl = cls(dfft.Configurations(), comm, precision=precision, rank=r)
            if chunks is not None:
                pl.setPipelineChunks(chunks)
            for k, v in (options or {}).items():
                pl.setOption(k, v)
            pl.initFFT(dfft.GlobalSize(*shape), dfft.Partition(P1, P2), allocate=False, c2c=c2c)
            self.plans.append(pl)
        self.C = self.plans[0].getPipelineChunks()
        self.nel = [pl.getDomainSize() // self.esz for pl in self.plans]
        # a work-area slice may be larger than the domain (padded private layouts of the single-rank z, x, y order)
        self.wel = [max(pl.getDomainSize(), pl.getWorkSizeDevice() // max(1, (self.P1 > 1) + (self.P2 > 1) + 1)) // self.esz for pl in self.plans]
        self.single = self.P == 1 and self.plans[0].debugPass("sz") is not None

    def buffers(self, n=3):
        return [[np.full(self.wel[r], np.nan + 0j, dtype=np.complex128) for _ in range(n)] for r in range(self.P)]

    def group(self, r, which):
        i, j = divmod(r, self.P2)
        return ([i * self.P2 + q for q in range(self.P2)], j) if which == 1 else ([q * self.P2 + j for q in range(self.P1)], i)

    def exchange(self, direction, which, c, send, recv):
        """all ranks: chunk c of exchange `which`; send/recv are per-rank flat complex arrays"""
        tabs = [pl.getPipelineTables(direction, which, c) for pl in self.plans]
        for r in range(self.P):
            grp, me = self.group(r, which)
            _, _, rc, rd = tabs[r]
            for q, peer in enumerate(grp):
                psc, psd, _, _ = tabs[peer]
                assert psc[me] == rc[q]
                n, e = rc[q] // self.esz, self.esz
                recv[r][rd[q] // e: rd[q] // e + n] = send[peer][psd[me] // e: psd[me] // e + n]

    def run(self, direction, ins, dims=3):
        """one exec of `dims` dimensions on every rank: the steps of the library's chain (dfft_debug_get_chain), each chunk of a step
        on every rank, then the exchange that follows it.  ins: per-rank flat input arrays (destroyed where the chain uses them as
        scratch); returns per-rank flat output arrays (complex after a forward exec, real after an R2C plan's inverse)"""
        steps = self.plans[0].debugChain(direction, dims)
        assert all(pl.debugChain(direction, dims) == steps for pl in self.plans[1:])
        if direction == dfft.FORWARD:
            outs = [np.full(n, np.nan + 0j, dtype=np.complex128) for n in self.nel]
        else:
            nin = [int(np.prod(pl.getInSize())) for pl in self.plans]
            outs = [np.full(n, np.nan, dtype=np.complex128 if self.c2c else np.float64) for n in nin]
        W = self.buffers(1 + max([0] + [b for s in steps for b in (s["src"], s["dst"])]))
        buf = lambda b: ins if b == -2 else outs if b == -1 else [W[r][b] for r in range(self.P)]
        length = (self.shape[2], self.shape[1], self.shape[0])      # by axis: z, y, x
        for i, s in enumerate(steps):
            src, dst, per = buf(s["src"]), buf(s["dst"]), s["per_chunk"]
            for c in range(s["launches"] // per):
                for r, pl in enumerate(self.plans):
                    for k in range(c * per, (c + 1) * per):
                        p = Pass(pl, s["group"], k)
                        if s["conj"]:
                            p.d.swap = 1
                        p.run(src[r], dst[r], length[s["axis"]], MODES[s["form"]])
                if s["exchange"]:
                    self.exchange(direction, s["exchange"], c, dst, buf(steps[i + 1]["src"]))
        return outs

    def forward(self, ins):
        return self.run(dfft.FORWARD, ins)

    def inverse(self, spec):
        """spec: per-rank flat complex arrays in the output layout (destroyed); returns per-rank
        flat arrays in the input layout (real for R2C plans)"""
        return self.run(dfft.INVERSE, spec)

    def partial(self, ins, d, direction):
        """execR2C/execC2R(out, in, d) for d = 1, 2"""
        return self.run(direction, ins, d)
