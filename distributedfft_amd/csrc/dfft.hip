// dfft.hip -- the plan's initialisation (dfft_init), the chain executor with its two sinks, and the C ABI of libdfft_amd.so.  How an
// axis is planned and how one pass over it is launched is axis.hip; pass descriptors: pipeline.hip; tuners: tune.hip.
//
// Host-side counterpart of the reference's decomposition classes; each block cites what it
// replaces (paths relative to the reference repository):
//   ctor / comm handling     src/mpicufft.cpp:42-66
//   initFFT                  src/pencil/mpicufft_pencil_opt1.cpp:46-326
//   setWorkArea              src/pencil/mpicufft_pencil_opt1.cpp:329-387
//   execR2C / execC2R        src/pencil/mpicufft_pencil_opt1.cpp:1422-1519 / 1522-1600
//   slab (P2 == 1)           src/slab/default/mpicufft_slab_opt1.cpp:38-178, 683-783
//   single rank (fft3d)      src/pencil/mpicufft_pencil_opt1.cpp:132-135, 1434-1436
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "alloc.hpp"
#include "axis.hpp"
#include "host_common.hpp"

namespace dfft {

static thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }

}  // namespace dfft

using namespace dfft;

static void fill_tables(dfft_plan *p, const Launch &L, PassArgs &A)
{
    A.lseg = reinterpret_cast<const SegTable *>(static_cast<const char *>(p->tables_d) + L.ltab);
    A.sseg = reinterpret_cast<const SegTable *>(static_cast<const char *>(p->tables_d) + L.stab);
    A.lnseg = L.lseg.nseg; A.snseg = L.sseg.nseg;
    A.ltab = L.lent == SIZE_MAX ? nullptr : reinterpret_cast<const SegEntry *>(static_cast<const char *>(p->tables_d) + L.lent);
    A.stab = L.sent == SIZE_MAX ? nullptr : reinterpret_cast<const SegEntry *>(static_cast<const char *>(p->tables_d) + L.sent);
}

// the launches of one group on axis `axis` (0 = z, 1 = y, 2 = x) in line form `form` (LineForm); conj: with conjugation
static int launch(dfft_plan *p, const Launch &L, int form, int axis, bool conj, const char *in, char *out, hipStream_t stream)
{
    if (L.args.ntiles == 0) return 0;
    const Axis &ax = p->ax[axis];
    PassArgs A = L.args;
    A.in = in + L.in_off; A.out = out + L.out_off; A.tw = ax.tw; A.debug = p->opt.debug;
    if (conj) A.swap = 1;
    fill_tables(p, L, A);
    // real forms: real lines in / out (real_mode 1 R2C, 2 C2R), the Hermitian half of NK = N/2 + 1 points on the other side
    const int real_mode = form == FORM_REAL_Z1 || form == FORM_REAL_LINES ? 1 : form == FORM_REAL_Z2 ? 2 : 0;
    const size_t NK = real_mode ? ax.N / 2 + 1 : ax.N;
    if (real_mode && (form == FORM_REAL_LINES ? p->yreal_native : p->zreal_native)) {
        // packed kernels: N/2-point complex transform + split / merge; the z pass of an R2C plan (A/B configurations: real_variant),
        // the strided real lines of a Y_Then_ZX R2C plan
        A.tw2 = p->tw_zr;
        const bool z = form != FORM_REAL_LINES;
        const int M = (int)((z ? p->Nz : p->Ny) / 2), variant = z ? p->opt.real_variant : 0;
        const int r = kernels(p->prec).launch_real(M, real_mode, variant, A, stream);
        if (r != 0) return fail(r == -1 ? ERR_UNSUPPORTED : r, "real pass launch failed for length " + std::to_string(2 * M));
        return 0;
    }
    const int variant = form == FORM_FWD ? p->vfwd[axis] : form == FORM_INV ? p->vinv[axis] : 0;
    return launch_axis(p->prec, ax, A, variant, real_mode, NK, static_cast<char *>(p->work_d) + p->lv_off, p->lv_bytes, p->TL, stream);
}

// one launch of group xx (fft_spectral_kernel): forward x pass, the multiplier `op`, inverse x pass
// (acc: added to what `out` holds -- the accumulating instantiations: table forms and STORE_TILED_SAME only, checked here and nowhere
// below, the kernel libraries' launchers take both for granted)
static int launch_spectral(dfft_plan *p, const Launch &L, const dfft_spectral_op &op, bool acc, const char *in, char *out, hipStream_t stream)
{
    if (L.args.ntiles == 0) return 0;
    const size_t real = p->esz / 2;
    PassArgs A = L.args;
    A.in = in + L.in_off; A.out = out + L.out_off; A.tw = p->ax[2].tw; A.debug = 0;
    fill_tables(p, L, A);
    A.mkind = op.kind; A.mscale = op.scale; A.acc = acc ? 1 : 0;
    if (acc && (op.kind == 0 || A.store_kind != STORE_TILED_SAME)) return fail(ERR_UNSUPPORTED, "spectral_sum: no accumulating kernel for this launch");
    if (op.kind == 0) A.mult = static_cast<const char *>(op.mult) + L.mult_off * p->esz;
    else if (op.kind != 3) { A.mtx = op.ax; A.mty = static_cast<const char *>(op.ay) + L.ty_off * real; A.mtz = op.az; }
    if (op.kind >= 3) {      // the factor tables; cy starts at the chunk's first ky row like ay, in complex elements
        A.mcx = op.cx; A.mcy = op.cy ? static_cast<const char *>(op.cy) + L.ty_off * p->esz : nullptr; A.mcz = op.cz;
    }
    // powers of two: this library's kernels; mixed radix (option value 2): libdfft_amd_any.so -- as dfft_init found (spectral_kernel_for)
    const Kernels &K = kernels(p->prec);
    const int r = (p->spectral_kernel == SPECTRAL_CORE ? K.launch_spectral : K.launch_spectral_mixed)((int)p->Nx, A, stream);
    if (r == -1) return fail(ERR_UNSUPPORTED, "spectral_op: unsupported x length " + std::to_string(p->Nx));
    if (r != 0) return fail(r, std::string("kernel launch failed: ") + hipGetErrorString((hipError_t)r));
    return 0;
}

// `ready`: an event recorded when the send data was complete (the producer kernel of this pipeline chunk), if the caller has one:
// the relay orders its first hop after it instead of after everything on `stream` (comm.hpp)
static int exchange_tables(dfft_plan *p, int which, const A2A &T, bool forward, const char *send, char *recv,
                           hipStream_t stream, int channel, uint64_t tag = 0, hipEvent_t ready = nullptr)
{
    const bool first = which == 1;
    const std::vector<int> &grp = first ? p->group1 : p->group2;
    const int me = first ? p->pj : p->pi;
    if (!p->comm) return fail(ERR_STATE, "exchange without a communicator");
    // Two-hop relay (comm.hpp): a group that is a strict subset of the world leaves most xGMI links idle -- the column groups of
    // a 2 x 4 grid drive one link of seven.  Option "relay" of the communicator: bit 0 = exchange 2, bit 1 = exchange 1.
    if ((p->comm->relay & (first ? 2 : 1)) && grp.size() > 1 && (int)grp.size() < p->comm->nranks) {
        if (!p->relay) p->relay = relay_cache_new();
        if (!tag) tag = (uint64_t)(uintptr_t)&T;      // the pipeline's tables live as long as the plan's initialisation
        const int r = forward ? relay_alltoallv(p->comm, p->relay, tag, p->rank, send, T.sc.data(), T.sd.data(), recv, T.rc.data(), T.rd.data(),
                                                grp.data(), (int)grp.size(), me, stream, channel, ready)
                              : relay_alltoallv(p->comm, p->relay, tag, p->rank, send, T.rc.data(), T.rd.data(), recv, T.sc.data(), T.sd.data(),
                                                grp.data(), (int)grp.size(), me, stream, channel, ready);
        return r ? fail(r, "relay exchange failed: " + g_error) : 0;
    }
    // the inverse all-to-all swaps the send and receive tables (mpicufft_pencil_opt1.cpp:829-830)
    p->comm->counters.alltoallv++;
    if (forward)
        return p->comm->alltoallv(p->rank, send, T.sc.data(), T.sd.data(), recv, T.rc.data(), T.rd.data(), grp.data(),
                                  (int)grp.size(), me, stream, channel);
    return p->comm->alltoallv(p->rank, send, T.rc.data(), T.rd.data(), recv, T.sc.data(), T.sd.data(), grp.data(),
                              (int)grp.size(), me, stream, channel);
}

static int exchange(dfft_plan *p, int which, bool forward, const void *send, void *recv)
{
    A2A T;
    T.sc = which == 1 ? p->sc1 : p->sc2; T.sd = which == 1 ? p->sd1 : p->sd2;
    T.rc = which == 1 ? p->rc1 : p->rc2; T.rd = which == 1 ? p->rd1 : p->rd2;
    // (the table is a temporary: name it by what it is -- exchange and direction)
    return exchange_tables(p, which, T, forward, static_cast<const char *>(send), static_cast<char *>(recv), p->stream, 0,
                           16 + 2 * (uint64_t)which + (forward ? 1 : 0));
}

// ---- per-phase timing: (start, stop) event pairs on whatever stream the work runs on --------
static int span_begin(dfft_plan *p, int phase, hipStream_t s)
{
    if (!p->timing) return 0;
    if (p->nspans == p->spans.size()) p->spans.emplace_back();
    TimedSpan &t = p->spans[p->nspans];
    if (!t.a) { HIP_TRY(hipEventCreate(&t.a)); HIP_TRY(hipEventCreate(&t.b)); }
    t.phase = phase; t.used = true;
    HIP_TRY(hipEventRecord(t.a, s));
    return 0;
}
static int span_end(dfft_plan *p, hipStream_t s)
{
    if (!p->timing) return 0;
    HIP_TRY(hipEventRecord(p->spans[p->nspans].b, s));
    p->nspans++;
    return 0;
}

// compute streams the chunked passes of this plan run on (Options::compute_streams)
static int compute_streams_of(const dfft_plan *p)
{
    const int C = p->pl.C, want = p->opt.compute_streams;
    if (C < 2) return 1;
    return want < 0 ? (C >= 3 ? 2 : 1) : (want > 1 ? 2 : 1);
}

static hipEvent_t pipe_event(dfft_plan *p, size_t i)
{
    Pipeline &pl = p->pl;
    while (pl.ev.size() <= i) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        pl.ev.push_back(e);
    }
    return pl.ev[i];
}

// the chain an exec of `dims` dimensions (3: the whole transform) in `direction` runs now
static const Chain &chain_of(const dfft_plan *p, int direction, int dims)
{
    const Pipeline &pl = p->pl;
    if (direction == DFFT_SPECTRAL_OP) return pl.spec;      // (dfft_exec_spectral_op; empty without option spectral_op)
    if (direction == DFFT_SPECTRAL_OPS) return pl.spec_multi;      // (dfft_exec_spectral_ops; empty while option spectral_outputs is 1)
    if (direction == DFFT_SPECTRAL_SUM) return pl.spec_sum;        // (dfft_exec_spectral_sum; empty while option spectral_inputs is 1)
    const bool fwd = direction != DFFT_INVERSE;
    if (dims == 3 && one_rank_alternative(p) && !(fwd ? pl.one_fwd : pl.one_inv).steps.empty()) return fwd ? pl.one_fwd : pl.one_inv;
    return fwd ? pl.fwd[dims - 1] : pl.inv[dims - 1];
}

std::vector<Launch> *pass_launches(dfft_plan *p, int k)
{
    // the z, x, y order of a single rank names its z / y / x passes fz / fy / fx, and its inverse runs them again
    static const int alt[6] = {G_SZ, G_SY, G_SX, -1, -1, -1};
    const int g = p->pl.single && one_rank_alternative(p) ? alt[k] : k;      // (G_FZ .. G_IZ == 0 .. 5)
    return g < 0 ? nullptr : &p->pl.groups[g].L;
}

// true where run_graphed replays (or is about to capture) the launches of an exec as one hipGraph: it captures the plan's stream alone
static bool graph_replay(const dfft_plan *p) { return p->opt.graph && p->nranks == 1 && !p->timing && (p->stream || !p->stream_user); }

// a launch of this line form on this axis goes through the plan's shared level scratch (two-level and long-Bluestein lines: launch())
static bool through_level_scratch(const dfft_plan *p, int form, int axis)
{
    const Axis &ax = p->ax[axis];
    const bool real = form == FORM_REAL_Z1 || form == FORM_REAL_Z2 || form == FORM_REAL_LINES;
    if (real && (form == FORM_REAL_LINES ? p->yreal_native : p->zreal_native)) return false;      // packed real kernels
    return ax.bluestein && (ax.longb || ax.two);
}

// The streams of an exec, as dfft_trace_op::stream numbers them, and which of them beside the plan's own an exec of chain `ch` uses:
// a predicate of the plan (options, chain, transport) shared by run_chain, the dry trace and the stream creation
enum { S_MAIN = 0, S_COMPUTE2 = 1, S_COMM = 2, S_COMM2 = 3 };
struct StreamUse { bool compute2, comm, comm2; };
static StreamUse streams_of(const dfft_plan *p, const Chain &ch)
{
    StreamUse u{};
    bool ex2 = false;
    for (const Step &s : ch.steps) ex2 = ex2 || s.xchg == 2;
    // two compute streams: never while two-level passes share one scratch, never under a graph capture of the plan's stream
    u.compute2 = ch.split && compute_streams_of(p) > 1 && !p->lv_bytes && !graph_replay(p);
    u.comm = p->comm && p->nranks > 1 && ch.steps.size() > 1;
    u.comm2 = u.comm && ex2 && p->P1 > 1 && p->P2 > 1 && p->comm->concurrent_channels();
    return u;
}

// ---- the leaf actions of run_chain go through a sink: HipSink issues them (and lists them under option trace), DrySink only lists
// them (dfft_debug_trace_chain).  Both build their records with the same functions.
static dfft_trace_op trace_launch(const dfft_plan *p, const std::vector<Step> &st, int step, int chunk, int k, int stream)
{
    const Step &t = st[(size_t)step];
    const Group &g = p->pl.groups[t.group];
    const int scratch = g.L[(size_t)k].args.ntiles != 0 && through_level_scratch(p, t.form, g.axis);
    return {0, stream, -1, step, chunk, k, t.src, t.dst, 0, scratch};
}
static dfft_trace_op trace_exchange(const std::vector<Step> &st, int step, int chunk, int stream)
{
    const Step &t = st[(size_t)step];
    return {1, stream, -1, step, chunk, -1, t.dst, st[(size_t)step + 1].src, t.xchg, 0};
}
static dfft_trace_op trace_sync(int kind, int stream, int event) { return {kind, stream, event, -1, -1, -1, -1, -1, 0, 0}; }

struct DrySink {
    const dfft_plan *p;
    const std::vector<Step> &st;
    std::vector<dfft_trace_op> &ops;
    int kernel(int step, int chunk, int k, int s) { ops.push_back(trace_launch(p, st, step, chunk, k, s)); return 0; }
    int xchg(int step, int chunk, int s, int /*ready*/) { ops.push_back(trace_exchange(st, step, chunk, s)); return 0; }
    int record(int s, int e) { ops.push_back(trace_sync(2, s, e)); return 0; }
    int wait(int e, int s) { ops.push_back(trace_sync(3, s, e)); return 0; }
    int begin(int, int) { return 0; }
    int end(int) { return 0; }
};

struct HipSink {
    dfft_plan *p;
    const std::vector<Step> &st;
    int direction;
    void *out;
    const void *in;
    std::vector<dfft_trace_op> *log;      // option trace, else nullptr
    hipStream_t S[4];
    // the streams the exec uses; one that does not exist yet is created here
    int open(const StreamUse &use)
    {
        Pipeline &pl = p->pl;
        if (use.compute2 && !pl.compute_stream2) HIP_TRY(hipStreamCreateWithFlags(&pl.compute_stream2, hipStreamNonBlocking));
        if (use.comm && !pl.comm_stream) HIP_TRY(hipStreamCreateWithFlags(&pl.comm_stream, hipStreamNonBlocking));
        if (use.comm2 && !pl.comm_stream2) HIP_TRY(hipStreamCreateWithFlags(&pl.comm_stream2, hipStreamNonBlocking));
        S[S_MAIN] = p->stream; S[S_COMPUTE2] = pl.compute_stream2; S[S_COMM] = pl.comm_stream; S[S_COMM2] = pl.comm_stream2;
        return 0;
    }
    char *buf(int b) const
    {
        if (b <= buf_input(1)) return const_cast<char *>(static_cast<const char *>(p->ins[-b - 9]));      // input j >= 1 of a multi-input chain (buf_input)
        if (b < BUF_IN) return static_cast<char *>(p->outs[-b - 2]);      // output j >= 1 of a multi-output chain (buf_output)
        return b == BUF_IN ? const_cast<char *>(static_cast<const char *>(in)) : b == BUF_OUT ? static_cast<char *>(out)
                                                                               : static_cast<char *>(p->work_d) + (size_t)b * p->domainsize;
    }
    int kernel(int step, int chunk, int k, int s)
    {
        const Step &t = st[(size_t)step];
        const Group &g = p->pl.groups[t.group];
        if (log) log->push_back(trace_launch(p, st, step, chunk, k, s));
        if (t.group == G_XX)
            return launch_spectral(p, g.L[(size_t)k], p->ops[direction == DFFT_SPECTRAL_SUM ? spectral_input_of(step) : spectral_output_of(step)],
                                   t.form == FORM_FIXED_ACC, buf(t.src), buf(t.dst), S[s]);
        return launch(p, g.L[(size_t)k], t.form, g.axis, t.conj, buf(t.src), buf(t.dst), S[s]);
    }
    int xchg(int step, int chunk, int s, int ready)
    {
        const Step &t = st[(size_t)step];
        const Pipeline &pl = p->pl;
        const int dir = t.tables ? t.tables : direction;
        const std::vector<A2A> &T = dir == DFFT_INVERSE ? (t.xchg == 1 ? pl.i1 : pl.i2) : (t.xchg == 1 ? pl.f1 : pl.f2);
        if (log) log->push_back(trace_exchange(st, step, chunk, s));
        return exchange_tables(p, t.xchg, T[(size_t)chunk], true, buf(t.dst), buf(st[(size_t)step + 1].src), S[s], s == S_COMM2 ? 1 : 0, 0,
                               pl.ev[(size_t)ready]);      // (tables in send / receive order)
    }
    int record(int s, int e)
    {
        hipEvent_t ev = pipe_event(p, (size_t)e);
        if (!ev) return fail(1, "hipEventCreate failed");
        if (log) log->push_back(trace_sync(2, s, e));
        HIP_TRY(hipEventRecord(ev, S[s]));
        return 0;
    }
    int wait(int e, int s)
    {
        if (log) log->push_back(trace_sync(3, s, e));
        HIP_TRY(hipStreamWaitEvent(S[s], p->pl.ev[(size_t)e], 0));
        return 0;
    }
    int begin(int phase, int s) { return span_begin(p, phase, S[s]); }
    int end(int s) { return span_end(p, S[s]); }
};

// The schedule of one execution chain (Pipeline::fwd / inv / one_fwd / one_inv): the one place that decides which stream a launch or
// an exchange takes and which events order them.  Streams and events are numbers here (dfft_trace_op); the sink acts on them.
//  - chunk c of a step runs on compute stream c mod 2 where the chain may split and the plan uses two compute streams (streams_of:
//    never while two-level passes share their scratch); every other launch runs on the plan's stream
//  - the exchange after chunk c runs on the communication stream of that exchange (2: the second one where the transport has concurrent
//    channels) behind an event recorded after the chunk (the relay's `ready`: comm.hpp), and records the event its consumer waits for
//  - chunk c of a step waits for the exchange of chunk c before it, or -- `whole` -- for all of the step before: the last exchange
//    chunk (the communication stream is in order) and the other compute stream; steps that depend chunk by chunk without an exchange
//    between them run interleaved, chunk c of the second right behind chunk c of the first
//  - the communication streams start after the caller's prior work (entry fence), the caller's stream ends after the second compute stream
template <typename Sink> static int schedule_chain(const dfft_plan *p, const Chain &ch, const StreamUse &use, Sink &sk)
{
    const std::vector<Step> &st = ch.steps;
    const Pipeline &pl = p->pl;
    const int Sc = S_MAIN, Sc2 = S_COMPUTE2, Sm = S_COMM, Sm2 = use.comm2 ? S_COMM2 : S_COMM;
    const bool two = use.compute2;
    auto SC = [&](int c) { return (two && (c & 1)) ? Sc2 : Sc; };
    int nev = 0;     // events of this exec, in order of use
    auto record = [&](int s, int &e) -> int { e = nev++; return sk.record(s, e); };
    auto wait = [&](int e, int s) -> int { return sk.wait(e, s); };
    auto join = [&](int from, int to) -> int { int e; TRY(record(from, e)); return wait(e, to); };
    const bool comm = use.comm;
    bool ex2 = false;
    for (const Step &s : st) ex2 = ex2 || s.xchg == 2;
    int fence = -1;
    if (comm || two) TRY(record(Sc, fence));
    if (comm) { TRY(wait(fence, Sm)); if (ex2 && Sm2 != Sm) TRY(wait(fence, Sm2)); }
    if (two) TRY(wait(fence, Sc2));
    int xdone[MAXSEG];            // exchange of chunk c of the step before is complete
    int xprev = 0, xn = 0;        // ... which exchange that was (0: none), after how many chunks
    for (size_t s0 = 0, s1; s0 < st.size(); s0 = s1) {
        for (s1 = s0 + 1; s1 < st.size() && !st[s1].whole && !st[s1 - 1].xchg; s1++) {}      // steps [s0, s1) run interleaved
        const Step &first = st[s0];
        const int nchunk = (int)(pl.groups[first.group].L.size() / first.per_chunk);
        const bool spread = two && nchunk > 1;      // on both compute streams
        if (first.whole) {
            if (spread) {      // both compute streams have finished what they were given so far
                int a, b;
                TRY(record(Sc2, a)); TRY(record(Sc, b)); TRY(wait(a, Sc)); TRY(wait(b, Sc2));
            }
            if (xprev) { TRY(wait(xdone[xn - 1], Sc)); if (spread) TRY(wait(xdone[xn - 1], Sc2)); }
            if (two && !spread) TRY(join(Sc2, Sc));
        }
        for (int c = 0; c < nchunk; c++) {
            const int S = SC(c);
            if (!first.whole && xprev) TRY(wait(xdone[c], S));
            for (size_t i = s0; i < s1; i++) {
                const Step &t = st[i];
                if (t.phase >= 0) TRY(sk.begin(t.phase, S));
                for (int k = c * t.per_chunk; k < (c + 1) * t.per_chunk; k++) TRY(sk.kernel((int)i, c, k, S));
                if (t.phase >= 0) TRY(sk.end(S));
            }
            const Step &t = st[s1 - 1];
            if (t.xchg) {
                const int Sx = t.xchg == 1 ? Sm : Sm2;
                int ready;
                TRY(record(S, ready)); TRY(wait(ready, Sx));
                if (t.phase >= 0) TRY(sk.begin(t.phase + 1, Sx));
                TRY(sk.xchg((int)s1 - 1, c, Sx, ready));
                if (t.phase >= 0) TRY(sk.end(Sx));
                TRY(record(Sx, xdone[c]));
            }
        }
        xprev = st[s1 - 1].xchg; xn = nchunk;
        if (s1 == st.size() && spread) TRY(join(Sc2, Sc));      // the caller's stream follows the odd chunks
    }
    return 0;
}

static int trace_slot(int direction)
{
    return direction == DFFT_SPECTRAL_SUM ? 4 : direction == DFFT_SPECTRAL_OPS ? 3 : direction == DFFT_SPECTRAL_OP ? 2 : direction == DFFT_INVERSE ? 1 : 0;
}

// Runs one execution chain: schedule_chain through the sink that issues HIP calls.  `prefix`: the chain to run where it is not
// chain_of's (the first steps of Pipeline::spec_multi for fewer outputs than the plan was built for, spectral_sum_chain for fewer inputs)
static int run_chain(dfft_plan *p, int direction, int dims, void *out, const void *in, const Chain *prefix = nullptr)
{
    const Chain &ch = prefix ? *prefix : chain_of(p, direction, dims);
    if (ch.steps.empty())
        return direction == DFFT_SPECTRAL_OP ? fail(ERR_STATE, "plan was initialised without option spectral_op")
               : direction == DFFT_SPECTRAL_OPS ? fail(ERR_STATE, "set spectral_outputs before dfft_init")
               : direction == DFFT_SPECTRAL_SUM ? fail(ERR_STATE, "set spectral_inputs before dfft_init")
                                             : fail(ERR_UNSUPPORTED, "the Y_Then_ZX sequence is forward only (as in the reference)");
    const StreamUse use = streams_of(p, ch);
    p->nspans = 0; p->last_dir = direction == DFFT_INVERSE ? DFFT_INVERSE : DFFT_FORWARD;
    std::vector<dfft_trace_op> *log = nullptr;
    if (p->opt.trace) { log = &p->trace_log[trace_slot(direction)]; log->clear(); }
    HipSink sk{p, ch.steps, direction, out, in, log, {}};
    TRY(sk.open(use));
    return schedule_chain(p, ch, use, sk);
}

// ------------------------------------------------------------------------------------------
// hipGraph replay (option "graph", off by default).  A single-rank exec is a handful of kernel launches on one stream.
// The first exec with a given (operation, in, out) runs plainly (lazy per-kernel attribute setup stays outside any
// capture), the second is captured into a graph, later ones replay it with one hipGraphLaunch.  Anything that changes the
// launches (dfft_init, dfft_set_work_area, dfft_set_stream, options, phase timing) drops the cached graphs.
// Measured on ROCm 7.2 / MI355X the replay is 6-8 us SLOWER per exec than the three plain launches it replaces
// (profiles/r2_graph_latency.txt), so it is not the default; it stays for callers that submit from a congested host thread.
// ------------------------------------------------------------------------------------------
void graphs_clear(dfft_plan *p)
{
    for (auto &g : p->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    p->graphs.clear();
}
template <typename F> static int run_graphed(dfft_plan *p, int kind, const void *in, void *out, F &&enqueue)
{
    if (!graph_replay(p) || !p->stream) return enqueue();
    dfft_plan::GraphEntry *e = nullptr;
    for (auto &g : p->graphs) if (g.kind == kind && g.in == in && g.out == out) { e = &g; break; }
    if (e && e->exec) { HIP_TRY(hipGraphLaunch(e->exec, p->stream)); return 0; }
    if (!e) {
        if (p->graphs.size() >= 16) graphs_clear(p);
        p->graphs.push_back({kind, in, out, 0, nullptr});
        e = &p->graphs.back();
    }
    if (e->uses < 0 || ++e->uses < 2) return enqueue();
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(p->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        e->uses = -1;                      // this stream cannot be captured: plain launches from now on
        return enqueue();
    }
    const int r = enqueue();
    const hipError_t ce = hipStreamEndCapture(p->stream, &graph);
    hipGraphExec_t exec = nullptr;
    if (r == 0 && ce == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
        (void)hipGraphDestroy(graph);
        e->exec = exec;
        HIP_TRY(hipGraphLaunch(exec, p->stream));
        return 0;
    }
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    e->uses = -1;
    if (r != 0) return r;                  // the enqueue itself failed: report that
    return enqueue();                      // nothing ran during the failed capture
}

int check_ready(dfft_plan *p)
{
    if (!p) return fail(ERR_ARG, "null plan");
    if (!p->initialized) return fail(ERR_STATE, "plan not initialised (call dfft_init first)");
    if (!p->work_d) return fail(ERR_STATE, "no work area (call dfft_set_work_area)");
    return 0;
}

static int ensure_device_state(dfft_plan *p);

// environment defaults of the user-facing knobs, read once per plan (never on the execution path)
static void env_defaults(Options &o)
{
    auto geti = [](const char *name, int &dst) { if (const char *v = getenv(name)) dst = atoi(v); };
    geti("DFFT_CHUNKS", o.chunks);
    geti("DFFT_TABLES", o.tables);
    geti("DFFT_SHIFT", o.shift);
    geti("DFFT_MIRROR", o.mirror);
    geti("DFFT_SINGLE_ORDER", o.single_order);
}

extern "C" {

const char *dfft_last_error(void) { return g_error.c_str(); }
const char *dfft_version(void) { return "distributedfft_amd 0.1 (gfx950)"; }

int dfft_comm_create_local(int nranks, dfft_comm **world)
{
    if (nranks < 1 || !world) return fail(ERR_ARG, "bad arguments");
    *world = make_local_world(nranks);
    return 0;
}
int dfft_rccl_unique_id(void *id128) { return rccl_unique_id(id128); }
int dfft_comm_create_rccl(const void *id128, int nranks, int rank, dfft_comm **comm)
{
    if (!id128 || !comm || rank < 0 || rank >= nranks) return fail(ERR_ARG, "bad arguments");
    *comm = make_rccl_comm(id128, nranks, rank);
    return *comm ? 0 : 1;
}
int dfft_comm_create_callback(int nranks, int rank, dfft_alltoallv_fn fn, void *user, dfft_comm **comm)
{
    if (!fn || !comm || rank < 0 || rank >= nranks) return fail(ERR_ARG, "bad arguments");
    *comm = make_callback_comm(nranks, rank, (void *)fn, user);
    return 0;
}
int dfft_comm_info(const dfft_comm *comm, int *nranks, int *transport_nranks)
{
    if (!comm) return fail(ERR_ARG, "null communicator");
    if (nranks) *nranks = comm->nranks;
    if (transport_nranks) *transport_nranks = comm->transport_nranks();
    return 0;
}
int dfft_comm_set_list_callback(dfft_comm *comm, dfft_sendrecv_list_fn fn, void *user)
{
    if (!comm) return fail(ERR_ARG, "null communicator");
    return callback_comm_set_list(comm, (void *)fn, user) ? fail(ERR_ARG, g_error) : 0;
}
int dfft_comm_get_counter(const dfft_comm *comm, const char *name, long *value)
{
    if (!comm || !name || !value) return fail(ERR_ARG, "null argument");
    const std::string k(name);
    if (k == "alltoallv") *value = comm->counters.alltoallv;
    else if (k == "list") *value = comm->counters.list;
    else if (k == "relayed") *value = comm->counters.relayed;
    else if (k == "relay_meta") *value = comm->counters.relay_meta;
    else if (k == "layered") *value = comm->counters.layered;
    else if (k == "relay_agree") *value = comm->counters.relay_agree;
    else return fail(ERR_ARG, "unknown counter " + k + " (alltoallv, list, relayed, relay_meta, relay_agree, layered)");
    return 0;
}
int dfft_comm_set_option(dfft_comm *comm, const char *key, long value)
{
    if (!comm || !key) return fail(ERR_ARG, "null communicator or key");
    if (std::string(key) == "relay") {      // handled above the transports (comm.hpp): every transport can relay
        if (value < 0 || value > 3) return fail(ERR_ARG, "relay: 0 off, 1 = exchange 2 (column groups), 2 = exchange 1 (row groups), 3 = both");
        comm->relay = (int)value;
        return 0;
    }
    if (std::string(key) == "test_channel") {
        if (value < 0 || value > 3) return fail(ERR_ARG, "test_channel: 0 .. 3");
        comm->test_channel = (int)value;
        return 0;
    }
    if (std::string(key) == "relay_overlap") {
        if (value < 0 || value > 1) return fail(ERR_ARG, "relay_overlap: 0 or 1");
        comm->relay_overlap = (int)value;
        return 0;
    }
    const int r = comm->set_option(key, value);
    if (r == 1 && g_error.empty()) set_error(std::string("this transport has no option ") + key);
    return r;
}
int dfft_comm_alltoallv(dfft_comm *comm, int myrank, const void *send, const size_t *scounts, const size_t *sdispls, void *recv,
                        const size_t *rcounts, const size_t *rdispls, const int *group, int ngroup, int me, void *hip_stream)
{
    if (!comm || !send || !recv || !scounts || !sdispls || !rcounts || !rdispls || !group) return fail(ERR_ARG, "null argument");
    if (ngroup < 1 || me < 0 || me >= ngroup) return fail(ERR_ARG, "bad group");
    comm->counters.alltoallv++;
    const int r = comm->alltoallv(myrank, send, scounts, sdispls, recv, rcounts, rdispls, group, ngroup, me, (hipStream_t)hip_stream, comm->test_channel);
    return r ? fail(r, "all-to-all failed: " + g_error) : 0;
}
int dfft_comm_sendrecv_list(dfft_comm *comm, int myrank, int nsend, const int *speer, const int *slayer, void *const *sptr, const size_t *sbytes,
                            int nrecv, const int *rpeer, const int *rlayer, void *const *rptr, const size_t *rbytes, int nlayers, void *hip_stream)
{
    if (!comm || nsend < 0 || nrecv < 0 || nlayers < 0) return fail(ERR_ARG, "bad arguments");
    if ((nsend && (!speer || !slayer || !sptr || !sbytes)) || (nrecv && (!rpeer || !rlayer || !rptr || !rbytes))) return fail(ERR_ARG, "null list");
    std::vector<dfft_xfer> sx((size_t)nsend), rx((size_t)nrecv);
    for (int i = 0; i < nsend; i++) {
        if (speer[i] < 0 || speer[i] >= comm->nranks || slayer[i] < 0 || slayer[i] >= nlayers) return fail(ERR_ARG, "send piece: bad peer or layer");
        sx[i] = dfft_xfer{speer[i], slayer[i], sptr[i], sbytes[i]};
    }
    for (int i = 0; i < nrecv; i++) {
        if (rpeer[i] < 0 || rpeer[i] >= comm->nranks || rlayer[i] < 0 || rlayer[i] >= nlayers) return fail(ERR_ARG, "receive piece: bad peer or layer");
        rx[i] = dfft_xfer{rpeer[i], rlayer[i], rptr[i], rbytes[i]};
    }
    const int r = comm->sendrecv_list(myrank, sx.data(), nsend, rx.data(), nrecv, nlayers, (hipStream_t)hip_stream, comm->test_channel);
    return r ? fail(r, "send/receive schedule failed: " + g_error) : 0;
}
int dfft_comm_destroy(dfft_comm *comm)
{
    delete comm;
    return 0;
}

int dfft_plan_create(dfft_plan **plan, int kind, int precision, const dfft_config *config, dfft_comm *comm,
                     int rank, int max_world_size)
{
    if (!plan) return fail(ERR_ARG, "null plan pointer");
    if (kind < DFFT_SLAB || kind > DFFT_SLAB_Y_THEN_ZX) return fail(ERR_ARG, "unknown plan kind");
    if (precision != DFFT_F32 && precision != DFFT_F64) return fail(ERR_ARG, "unknown precision");
    dfft_plan *p = new dfft_plan;
    p->kind = kind; p->prec = precision;
    if (config) p->cfg = *config;
    p->comm = comm;
    p->nranks = comm ? comm->nranks : 1;
    p->rank = comm ? (comm->fixed_rank() >= 0 ? comm->fixed_rank() : rank) : 0;
    // max_world_size: the reference truncates the communicator to the first ranks
    // (src/mpicufft.cpp:46-51); here ranks beyond it simply may not create plans.
    if (max_world_size > 0 && max_world_size < p->nranks) p->nranks = max_world_size;
    if (p->rank < 0 || p->rank >= p->nranks) { delete p; return fail(ERR_ARG, "rank outside the world"); }
    p->esz = kernels(precision).esz;
    p->TL = kernels(precision).TL;
    env_defaults(p->opt);
    *plan = p;
    return 0;
}

static const char *const kPassNames[6] = {"fz", "fy", "fx", "ix", "iy", "iz"};
static int *option_slot(Options &o, const std::string &k)
{
    if (k == "pipeline_chunks") return &o.chunks;
    if (k == "two_level") return &o.two_level;
    if (k == "mirror_inverse") return &o.mirror;
    if (k == "point_tables") return &o.tables;
    if (k == "uniform_tables") return &o.uniform_tables;
    if (k == "shift") return &o.shift;
    if (k == "debug_skip") return &o.debug;
    if (k == "real_variant") return &o.real_variant;
    if (k == "single_order") return &o.single_order;
    if (k == "single_layout") return &o.single_layout;
    if (k == "single_pad") return &o.single_pad;
    if (k == "native_mixed") return &o.native_mixed;
    if (k == "graph") return &o.graph;
    if (k == "spectral_layout") return &o.spectral;
    if (k == "spectral_op") return &o.spectral_op;
    if (k == "spectral_outputs") return &o.spectral_outputs;
    if (k == "spectral_inputs") return &o.spectral_inputs;
    if (k == "compute_streams") return &o.compute_streams;
    if (k == "trace") return &o.trace;
    for (int i = 0; i < 6; i++) {
        if (k == std::string("variant_") + kPassNames[i]) return &o.variant[i];
        if (k == std::string("order_") + kPassNames[i]) return &o.order[i];
    }
    return nullptr;
}
int dfft_set_option(dfft_plan *p, const char *key, long value)
{
    if (!p || !key) return fail(ERR_ARG, "null plan or key");
    int *slot = option_slot(p->opt, key);
    if (!slot) return fail(ERR_ARG, std::string("unknown option ") + key);
    // kernel configurations are keyed by (length, variant) with four bits for the variant (kernels.hip.inc)
    if (std::string(key).rfind("variant_", 0) == 0 && (value < -1 || value > 15)) return fail(ERR_ARG, "variant_* must be -1 (the plan's choice) or 0..15");
    *slot = (int)value;      // takes effect at the next dfft_init (debug_skip / mirror_inverse / real_variant: next exec)
    graphs_clear(p);         // captured launches carry the old options
    return 0;
}
long dfft_get_option(dfft_plan *p, const char *key)
{
    if (!p || !key) return -1;
    int *slot = option_slot(p->opt, key);
    return slot ? *slot : -1;
}

int dfft_plan_destroy(dfft_plan *p)
{
    if (!p) return 0;
    graphs_clear(p);
    if (p->work_owned && p->work_d) (void)dev_free(p->work_d);
    relay_cache_free(p->relay);
    for (auto &a : p->ax) axis_free(a);
    for (void *t : {p->tw_zr, p->tables_d}) if (t) (void)hipFree(t);
    for (auto &t : p->spans) { if (t.a) (void)hipEventDestroy(t.a); if (t.b) (void)hipEventDestroy(t.b); }
    for (auto &e : p->pl.ev) if (e) (void)hipEventDestroy(e);
    if (p->pl.comm_stream) (void)hipStreamDestroy(p->pl.comm_stream);
    if (p->pl.comm_stream2) (void)hipStreamDestroy(p->pl.comm_stream2);
    if (p->pl.compute_stream2) (void)hipStreamDestroy(p->pl.compute_stream2);
    if (p->stream_owned && p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
    return 0;
}

// axis plans: native chain (powers of two 2..8192, mixed-radix lengths up to 2048) or Bluestein (any length with 2N-1 <= 8192)
static int plan_axes(dfft_plan *p, size_t Nx, size_t Ny, size_t Nz, bool c2c, bool yzx)
{
    Axis az, ay, axx;
    const bool mixed = p->opt.native_mixed != 0;
    // packed real z pass: Nz/2-point complex transform + Hermitian split / merge (powers of two, and even lengths whose
    // half has a mixed-radix configuration)
    const int tl = p->opt.two_level;      // 1: two-level lines wherever a split exists (the packed real kernels then stand back)
    const bool zr_native = !yzx && !c2c && tl != 1 && Nz >= 4 && Nz <= 4096 && Nz % 2 == 0 && (is_pow2(Nz) || mixed) &&
                           kernels(p->prec).real_supported((int)(Nz / 2));
    const size_t zlen = zr_native ? Nz / 2 : Nz;
    // Y_Then_ZX, R2C: the y pass reads real lines in place, which only the Bluestein kernel does
    // Y_Then_ZX, R2C: the y pass reads real lines in place.  Power-of-two Ny: the packed Ny/2-point real kernel
    // with its strided-line load; any other Ny: the Bluestein kernel's real mode (Ny <= 4096)
    const bool yr_native = yzx && !c2c && tl != 1 && is_pow2(Ny) && Ny >= 4 && Ny <= 2048;
    const bool yok = yr_native ? axis_plan(p->prec, Ny / 2, ay) : yzx && !c2c ? axis_plan_bluestein(p->prec, Ny, ay, tl) : axis_plan(p->prec, Ny, ay, mixed, tl);
    // a real z pass is either the packed Nz/2-point kernel or the Bluestein kernel's real modes: never
    // the plain complex chain (Nz == 2 would otherwise pick it and launch Bluestein without its tables)
    const bool zreal_generic = !yzx && !c2c && !zr_native;
    const bool zok = zreal_generic ? axis_plan_bluestein(p->prec, Nz, az, tl) : axis_plan(p->prec, zlen, az, mixed, tl);
    if (!zok || !yok || !axis_plan(p->prec, Nx, axx, mixed, tl))
        return fail(ERR_UNSUPPORTED, "unsupported axis length (every length from 2 to 2^23 has a plan; beyond that only lengths N1*N2 <= 2^24 whose "
                                     "factors are each a power of two up to 8192 or any length up to 4096)");
    // an axis outside the power-of-two kernels of this library runs kernels of libdfft_amd_any.so (any_loader.hip): no fallback
    for (const Axis *a : {&az, &ay, &axx}) {
        std::string why;
        if ((a->bluestein || !is_pow2(a->N)) && !any_available(&why))
            return fail(ERR_UNSUPPORTED, "an axis of " + std::to_string(a->N) + " points needs the kernels of libdfft_amd_any.so (every length that is "
                                         "not a power of two up to 8192): " + why);
    }
    for (auto &a : p->ax) axis_free(a);
    p->ax[0] = az; p->ax[1] = ay; p->ax[2] = axx;
    p->zreal_native = zr_native;
    p->yreal_native = yr_native;
    return 0;
}

// option spectral_op: the plans that have the fused chain, and the fused x kernel the plan's x axis runs (p->spectral_kernel)
static int admit_spectral_op(dfft_plan *p, bool sequence)
{
    if (sequence && p->opt.spectral_op == 2)
        return fail(ERR_UNSUPPORTED, "spectral_op: no fused chain for the Z_Then_YX / Y_Then_ZX sequences, whatever the x length (" + std::to_string(p->Nx) +
                                     " points here): pencil and default slab plans only");
    if (sequence) return fail(ERR_UNSUPPORTED, "spectral_op: pencil and default slab plans only (not the Z_Then_YX / Y_Then_ZX sequences)");
    if (p->opt.spectral_op != 1 && p->opt.spectral_op != 2) return fail(ERR_ARG, "spectral_op: 0, 1 or 2");
    std::string why;
    p->spectral_kernel = spectral_kernel_for(p->prec, p->ax[2], p->opt.spectral_op, &why);
    return p->spectral_kernel == SPECTRAL_NONE ? fail(ERR_UNSUPPORTED, why) : 0;
}

// kernel configuration per pass, by role (PassRole); lengths without a configuration for a role use the default
static void choose_pass_roles(dfft_plan *p)
{
    auto has = [&](const Axis &a, int role) { return has_variant(p->prec, a, role); };
    for (int k = 0; k < 3; k++) p->vfwd[k] = p->vinv[k] = ROLE_DEFAULT;
    if (p->prec == DFFT_F64) {
        // the multi-rank inverse x pass reads the point-major API layout: 16 lines x 32 points (256-byte runs) -- where the rows
        // are whole tiles.  On the 513-wide rows of an R2C plan the 256-byte runs straddle three cache lines and the one
        // workgroup per CU re-reads 17 % of them (profiles/r3_pmc_traffic_f64_r2c.json): the default configuration (8 lines,
        // two workgroups per CU) is 15 % faster there, 3.66 vs 4.26 ms at 1024^3 (profiles/r3_strided_read_odd_pitch.txt)
        const size_t zs_local = p->zs.empty() ? p->Nzc : p->zs[p->zyx ? (size_t)p->rank % p->zs.size() : (size_t)p->pj % p->zs.size()];
        if (has(p->ax[2], ROLE_STRIDED_READ) && zs_local % (size_t)p->TL == 0) p->vinv[2] = ROLE_STRIDED_READ;
        // ... and without a second exchange (P1 = 1) its persistent form with stores and loads fused (8.27 -> 7.64 ms at 1024^3,
        // profiles/r4_persist3.txt); launches that do not have its pair of address forms run ROLE_STRIDED_READ by themselves
        if (p->vinv[2] == ROLE_STRIDED_READ && p->P1 == 1 && has(p->ax[2], ROLE_STRIDED_READ_FUSED)) p->vinv[2] = ROLE_STRIDED_READ_FUSED;
        // complex z passes have natural lines on one side and long-run stores
        const int zrole = has(p->ax[0], ROLE_LINES) ? ROLE_LINES : has(p->ax[0], ROLE_STREAM) ? ROLE_STREAM : ROLE_DEFAULT;
        if (p->c2c) p->vfwd[0] = p->vinv[0] = zrole;
        // the inverse y pass stores tiled-transpose chunks (1 KiB runs)
        if (has(p->ax[1], ROLE_STREAM)) p->vinv[1] = ROLE_STREAM;
        if (p->opt.spectral) {      // x passes with natural lines on one side, like the complex z passes
            const int xrole = has(p->ax[2], ROLE_LINES) ? ROLE_LINES : has(p->ax[2], ROLE_STREAM) ? ROLE_STREAM : ROLE_DEFAULT;
            p->vfwd[2] = p->vinv[2] = xrole;
        }
    } else {
        if (p->c2c && has(p->ax[0], ROLE_NATURAL_LOAD)) p->vfwd[0] = ROLE_NATURAL_LOAD;
        if (p->c2c && has(p->ax[0], ROLE_NATURAL_STORE)) p->vinv[0] = ROLE_NATURAL_STORE;
        for (int ax = 1; ax <= 2; ax++)
            if (has(p->ax[ax], ROLE_TILED)) p->vfwd[ax] = p->vinv[ax] = ROLE_TILED;
        // the inverse y pass of a multi-rank plan stores transposed tiles: whole-line stores (ROLE_TRANSPOSED_STORE) where the length
        // has such a configuration (2048 points: 4.80 -> 3.63 ms on rank 0 of 2 x 4 at 2048^3)
        // (a single rank's complex inverse runs the forward launches: there vinv is not used)
        if (has(p->ax[1], ROLE_TRANSPOSED_STORE)) p->vinv[1] = ROLE_TRANSPOSED_STORE;
        // 2048 points and more on a multi-rank plan: the forward y pass and the inverse x pass (the strided read of the API layout)
        // run the streaming sibling of the tiled configuration -- what dfft_tune_variants picked on every 2048^3 plan measured
        // (rank 0 of 2 x 4: y 4.93 -> 3.78 ms, x^-1 5.36 -> 4.46; of 8 x 1 the same two; profiles/r5_tuner_choices.txt).  The
        // forward x pass and the inverse y pass lose with it (round 3), shorter lines were not measured: they keep their rule.
        if (p->nranks > 1 && p->ax[1].N >= 2048 && has(p->ax[1], ROLE_TILED_STREAM)) p->vfwd[1] = ROLE_TILED_STREAM;
        if (p->nranks > 1 && p->ax[2].N >= 2048 && has(p->ax[2], ROLE_TILED_STREAM)) p->vinv[2] = ROLE_TILED_STREAM;
        if (p->opt.spectral) {      // x-contiguous spectrum: the forward x pass stores natural lines like the inverse z pass
            if (has(p->ax[2], ROLE_NATURAL_STORE)) p->vfwd[2] = ROLE_NATURAL_STORE;
            // ... and its inverse loads them: point fastest for the first pass only, the same-tile stores stay line fastest
            if (has(p->ax[2], ROLE_NATURAL_LOAD_TILED_STORE)) p->vinv[2] = ROLE_NATURAL_LOAD_TILED_STORE;
        }
        // (The inverse y pass stores transposed tiles, which a line-fastest fp32 wave -- 16 lines x 4 points -- writes in 32-byte
        // pieces.  A point-fastest store mapping, PassCfg::MAP = 2, writes whole lines and was measured: 1024 points 4.42 vs 4.30 ms,
        // 2048 points 10.55 vs 10.35, no better -- L2 merges the pieces; profiles/r3_f32_inverse_y_point_fastest_store.txt.)
    }
}

int dfft_init(dfft_plan *p, size_t Nx, size_t Ny, size_t Nz, int P1, int P2, int c2c, int allocate)
{
    if (!p) return fail(ERR_ARG, "null plan");
    p->initialized = false;      // a failed (re-)initialisation must not leave a half-updated plan executable
    graphs_clear(p);
    relay_cache_free(p->relay);      // gathered per exchange table: the tables are about to change
    p->relay = nullptr;
    if (!Nx || !Ny || !Nz) return fail(ERR_ARG, "GlobalSize not initialized!");
    if (P1 < 1 || P2 < 1 || P1 * P2 != p->nranks) return fail(ERR_ARG, "Invalid Input Partition!");
    const bool zyx_kind = p->kind == DFFT_SLAB_Z_THEN_YX || p->kind == DFFT_SLAB_Z_THEN_YX_OPT1;
    const bool yzx = p->kind == DFFT_SLAB_Y_THEN_ZX;
    if ((p->kind == DFFT_SLAB || p->kind == DFFT_SLAB_OPT1 || zyx_kind || yzx) && P2 != 1)
        return fail(ERR_ARG, "slab decomposition needs P2 == 1");
    // one rank: every class is the same local 3-D transform (fft3d branch, mpicufft_slab_z_then_yx.cpp:118-122)
    const bool zyx = zyx_kind && P1 > 1;
    if (P1 > MAXSEG || P2 > MAXSEG) return fail(ERR_UNSUPPORTED, "more than 32 ranks per exchange group");
    if ((size_t)P1 > Nx || (!zyx && (size_t)P1 > Ny) || (size_t)P2 > Ny) return fail(ERR_ARG, "partition larger than the grid");
    TRY(plan_axes(p, Nx, Ny, Nz, c2c != 0, yzx));
    p->Nx = Nx; p->Ny = Ny; p->Nz = Nz; p->c2c = c2c != 0;
    p->Nzc = (c2c || yzx) ? Nz : Nz / 2 + 1;
    p->Nyc = (yzx && !c2c) ? Ny / 2 + 1 : Ny;      // Hermitian axis y (mpicufft_slab_y_then_zx.cpp:96-104)
    if ((size_t)P2 > p->Nzc || (zyx && (size_t)P1 > p->Nzc)) return fail(ERR_ARG, "partition larger than the grid");
    p->zyx = zyx; p->yzx = yzx;
    if (yzx && (size_t)P1 > p->Nyc) return fail(ERR_ARG, "partition larger than the grid");
    p->P1 = P1; p->P2 = P2;
    p->pi = p->rank / P2; p->pj = p->rank % P2;       // pidx = pidx_i * P2 + pidx_j (:67-68)
    split(Nx, P1, p->xs, p->xstart);
    split(Ny, P2, p->ys, p->ystart);
    // Z_Then_YX: the output is split along z over all ranks (mpicufft_slab_z_then_yx.cpp:96-103)
    split(p->Nzc, zyx ? P1 : P2, p->zs, p->zstart);
    split(p->Nyc, P1, p->yo, p->yostart);
    const size_t xs = p->xs[p->pi], ys = p->ys[p->pj], zs = p->zs[zyx ? p->pi : p->pj], yo = p->yo[p->pi];
    // domainsize = largest stage (:203-209)
    p->domain_elems = zyx ? std::max(xs * Ny * p->Nzc, Nx * Ny * zs)
                      : yzx ? std::max(xs * p->Nyc * Nz, Nx * yo * Nz)
                            : std::max({xs * ys * p->Nzc, xs * Ny * zs, Nx * yo * zs});
    p->domainsize = p->domain_elems * p->esz;
    p->domainsize = (p->domainsize + 255) & ~(size_t)255;
    const int nexch = (P1 > 1) + (P2 > 1);
    p->worksize_d = p->domainsize * (size_t)(nexch + 1);   // one slice per exchange + 1
    // all-to-all tables in bytes (:269-273, :315-319)
    const size_t e = p->esz;
    p->sc1.assign(P2, 0); p->sd1.assign(P2, 0); p->rc1.assign(P2, 0); p->rd1.assign(P2, 0);
    p->group1.assign(P2, 0);
    for (int q = 0; q < P2; q++) {
        p->sc1[q] = e * p->zs[q] * ys * xs;
        p->sd1[q] = e * p->zstart[q] * ys * xs;
        p->rc1[q] = e * xs * p->ys[q] * zs;
        p->rd1[q] = e * xs * p->ystart[q] * zs;
        p->group1[q] = p->pi * P2 + q;
    }
    p->sc2.assign(P1, 0); p->sd2.assign(P1, 0); p->rc2.assign(P1, 0); p->rd2.assign(P1, 0);
    p->group2.assign(P1, 0);
    for (int q = 0; q < P1; q++) {
        if (zyx) {      // mpicufft_slab_z_then_yx.cpp:190-196
            p->sc2[q] = e * p->zs[q] * Ny * xs;
            p->sd2[q] = e * p->zstart[q] * Ny * xs;
            p->rc2[q] = e * zs * Ny * p->xs[q];
            p->rd2[q] = e * zs * Ny * p->xstart[q];
        } else {
            p->sc2[q] = e * xs * zs * p->yo[q];
            p->sd2[q] = e * xs * zs * p->yostart[q];
            p->rc2[q] = e * p->xs[q] * yo * zs;
            p->rd2[q] = e * p->xstart[q] * yo * zs;
        }
        p->group2[q] = q * P2 + p->pj;
    }
    // pipeline depth: chunks of the outer axis exchanged while the next chunk is transformed
    {
        int C = p->opt.chunks;
        if (C <= 0) C = nexch ? 4 : 1;
        size_t lim = (size_t)MAXSEG / (size_t)P1;            // segments of the x / ky axis = P1 * C
        for (int q = 0; q < P1; q++) lim = std::min({lim, p->xs[q], zyx ? p->xs[q] : p->yo[q]});
        if ((size_t)C > lim) C = (int)lim;
        if (C < 1) C = 1;
        p->pl.C = C;
    }
    if (p->opt.spectral && (zyx || yzx)) return fail(ERR_UNSUPPORTED, "spectral_layout: pencil and default slab plans only (not the Z_Then_YX / Y_Then_ZX sequences)");
    if (p->opt.spectral && p->opt.spectral != 1) return fail(ERR_ARG, "spectral_layout: 0 = the reference's [Nx][yo][zs], 1 = x-contiguous [yo][zs][Nx]");
    if (p->opt.spectral_op) {
        TRY(admit_spectral_op(p, zyx || yzx));
        p->worksize_d += p->domainsize;      // the slice that stands in for `out` (forward half) and `in` (inverse half)
    }
    if (p->opt.spectral_outputs < 1 || p->opt.spectral_outputs > DFFT_SPECTRAL_MAX_OUTPUTS)
        return fail(ERR_ARG, "spectral_outputs: 1 to " + std::to_string(DFFT_SPECTRAL_MAX_OUTPUTS));
    if (p->opt.spectral_outputs > 1) {
        if (!p->opt.spectral_op) return fail(ERR_ARG, "spectral_outputs: needs option spectral_op = 1 or 2");
        // the multi-output chain never writes the slice xx reads: one more slice wherever the single-output chain writes it again
        // (every grid but a P1 x P2 pencil: pipeline.hip), whatever the number of outputs
        if (P1 == 1 || P2 == 1) p->worksize_d += p->domainsize;
    }
    if (p->opt.spectral_inputs < 1 || p->opt.spectral_inputs > DFFT_SPECTRAL_MAX_INPUTS)
        return fail(ERR_ARG, "spectral_inputs: 1 to " + std::to_string(DFFT_SPECTRAL_MAX_INPUTS));
    if (p->opt.spectral_inputs > 1) {
        if (!p->opt.spectral_op) return fail(ERR_ARG, "spectral_inputs: needs option spectral_op = 1 or 2");
        // the accumulator of the multi-input chain: one slice above the single chain's on every grid, whatever the number of inputs.  The
        // multi-output chain's extra slice has the same index and the two chains never run at the same time: a plan pays for it once
        if (!(p->opt.spectral_outputs > 1 && (P1 == 1 || P2 == 1))) p->worksize_d += p->domainsize;
    }
    // (one rank: the inverse of an x-contiguous spectrum cannot be the forward launches with conjugation -- their input is the natural grid)
    p->spectral_mirror = p->opt.spectral && p->nranks == 1;
    TRY(zyx ? build_pipeline_zyx(p, p->pl) : yzx ? build_pipeline_yzx(p, p->pl) : build_pipeline(p, p->pl));
    TRY(build_pipeline_single(p, p->pl));
    if (p->pl.single) {
        const size_t need = (p->pl.single_work_elems * p->esz + 255) & ~(size_t)255;
        p->worksize_d = std::max(p->worksize_d, need);      // the padded L2 buffer lives in the work area
    }
    {   // two-level axes: the scratch between the levels is a region of the work area behind the exchange slices, sized for the
        // largest launch (tiles x TL lines x N points)
        size_t lvb = 0;
        for (const Group &g : p->pl.groups)
            for (const Launch &L : g.L) lvb = std::max(lvb, axis_scratch_bytes(p->prec, p->ax[g.axis], L.args, p->TL));
        p->worksize_d = (p->worksize_d + 255) & ~(size_t)255;
        p->lv_off = p->worksize_d;
        p->lv_bytes = (lvb + 255) & ~(size_t)255;
        p->worksize_d += p->lv_bytes;
    }
    choose_pass_roles(p);
    for (int k = 0; k < 6; k++) {      // per-pass overrides (dfft_set_option): fz fy fx ix iy iz
        const int d = p->opt.order[k];
        if (std::vector<Launch> *v = d >= 0 ? pass_launches(p, k) : nullptr)
            for (Launch &L : *v) { L.args.a_fastest = d & 1; L.args.xcd_swizzle = (d >> 1) & 1; }
        if (p->opt.variant[k] >= 0) (k < 3 ? p->vfwd[k] : p->vinv[5 - k]) = p->opt.variant[k];
    }
    for (auto &a : p->ax) axis_free(a);
    for (void **t : {&p->tw_zr, &p->tables_d}) if (*t) { (void)hipFree(*t); *t = nullptr; }
    p->initialized = true;
    // device-side state (twiddles, stream, work area) is created by setWorkArea, so that the
    // decomposition tables can be queried on a host without a GPU (allocate = 0).
    if (allocate) return dfft_set_work_area(p, nullptr, nullptr);
    return 0;
}

// per-point address tables (SegEntry, fft_pass.hip.h) of a launch's segmented side
static void point_table(const Launch &L, bool store, std::vector<SegEntry> &tab)
{
    const SegTable &T = store ? L.sseg : L.lseg;
    const PassArgs &A = L.args;
    size_t cover = 0;
    for (int s = 0; s < T.nseg; s++) cover = std::max(cover, (size_t)T.start[s] + T.len[s]);
    tab.assign(cover, SegEntry{0, 0, 0});
    for (size_t n = 0; n < cover; n++) {
        int s = 0;                      // same rule as the kernels: last segment whose start is <= n
        for (int q = 1; q < T.nseg; q++) if (n >= T.start[q]) s = q;
        const uint64_t d = n - T.start[s], ln = T.len[s];
        SegEntry e;
        e.ln = (uint32_t)ln;
        if (!store) {
            e.base = T.base[s]; e.aux = (uint32_t)d;
        } else if (A.store_kind == STORE_TILED_SAME) {
            e.base = T.base[s] + d * (A.SK ? A.SK : (uint64_t)A.LB * A.LA); e.aux = 0;
        } else {
            const uint64_t T2 = 1ull << A.T2shift, kt = d >> A.T2shift, kr = d & (T2 - 1);
            const uint64_t r2 = ln - kt * T2;
            e.base = T.base[s] + kt * T2 * A.LB + kr;
            e.aux = (uint32_t)std::min(r2, T2);
        }
        tab[n] = e;
    }
}

static int upload_tables(dfft_plan *p)
{
    Pipeline &pl = p->pl;
    // DFFT_TABLES: 0 = search the segment table per point, 1 = per-point tables for launches with
    // more than one segment (default), 2 = tables for every tiled load / store
    const int mode = p->opt.tables;
    std::vector<Launch *> all;
    for (Group &g : pl.groups) for (Launch &L : g.L) all.push_back(&L);
    std::vector<char> host(all.size() * 2 * sizeof(SegTable));
    size_t off = 0;
    for (Launch *L : all) {
        L->ltab = off; memcpy(host.data() + off, &L->lseg, sizeof(SegTable)); off += sizeof(SegTable);
        L->stab = off; memcpy(host.data() + off, &L->sseg, sizeof(SegTable)); off += sizeof(SegTable);
    }
    std::vector<SegEntry> tab;
    for (Launch *L : all) {
        L->lent = L->sent = SIZE_MAX;
        const bool tl = L->args.load_kind == LOAD_TILED && L->lseg.nseg >= 1;
        const bool ts = (L->args.store_kind == STORE_TILED_SAME || L->args.store_kind == STORE_TILED_TRANSPOSE) && L->sseg.nseg >= 1;
        for (int side = 0; side < 2; side++) {
            const bool want = side == 0 ? tl : ts;
            const int nseg = side == 0 ? L->lseg.nseg : L->sseg.nseg;
            if (!want || mode == 0 || (mode == 1 && nseg < 2) || L->args.ntiles == 0) continue;
            if ((side == 0 && L->args.IA) || (side == 1 && L->args.SK)) continue;      // explicit strides: closed form only
            point_table(*L, side == 1, tab);
            (side == 0 ? L->lent : L->sent) = host.size();
            // wave-uniform (scalar) table reads need the 4 / 8 / 16 consecutive points of a wave in one segment
            const SegTable &T = side == 0 ? L->lseg : L->sseg;
            bool aligned = p->opt.uniform_tables != 0;
            for (int q = 0; q < T.nseg; q++) aligned = aligned && T.start[q] % 16 == 0;
            (side == 0 ? L->args.luni : L->args.suni) = aligned ? 1 : 0;
            const size_t bytes = tab.size() * sizeof(SegEntry);
            host.resize(host.size() + bytes);
            memcpy(host.data() + host.size() - bytes, tab.data(), bytes);
        }
    }
    if (p->tables_d) { (void)hipFree(p->tables_d); p->tables_d = nullptr; }
    HIP_TRY(hipMalloc(&p->tables_d, host.size()));
    HIP_TRY(hipMemcpy(p->tables_d, host.data(), host.size(), hipMemcpyHostToDevice));
    return 0;
}

static int ensure_device_state(dfft_plan *p)
{
    if (!p->tables_d) TRY(upload_tables(p));
    for (auto &a : p->ax) TRY(axis_upload(p->prec, a));
    if (p->zreal_native && !p->tw_zr) TRY(make_twiddles(p->prec, p->Nz, &p->tw_zr));
    if (p->yreal_native && !p->tw_zr) TRY(make_twiddles(p->prec, p->Ny, &p->tw_zr));
    if (!p->stream && !p->stream_user) {
        HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
        p->stream_owned = true;
    }
    // the streams the whole transform needs as the options stand (an exec creates what it needs beyond them: HipSink::open)
    for (const Chain *ch : {&chain_of(p, DFFT_FORWARD, 3), &chain_of(p, DFFT_INVERSE, 3), &chain_of(p, DFFT_SPECTRAL_OP, 3)}) {
        HipSink sk{p, ch->steps, DFFT_FORWARD, nullptr, nullptr, nullptr, {}};
        TRY(sk.open(streams_of(p, *ch)));
    }
    return 0;
}

int dfft_set_work_area(dfft_plan *p, void *device, void *host)
{
    (void)host;   // no host staging: device buffers are handed to the transport directly
    if (!p) return fail(ERR_ARG, "null plan");
    if (!p->initialized) return fail(ERR_STATE, "cannot set work area: plan not initialised");
    graphs_clear(p);
    if (p->work_owned && p->work_d) { (void)dev_free(p->work_d); p->work_d = nullptr; p->work_owned = false; }
    TRY(ensure_device_state(p));
    if (device) {
        p->work_d = device;   // caller keeps ownership (:333-342)
    } else {
        TRY(dev_alloc_default(p->worksize_d, &p->work_d));      // (the virtual-memory backing: see default_chunk_mib)
        p->work_owned = true;
    }
    return 0;
}

int dfft_set_pipeline_chunks(dfft_plan *p, int chunks)
{
    if (!p) return fail(ERR_ARG, "null plan");
    if (chunks < 0) return fail(ERR_ARG, "chunks must be >= 0");
    p->opt.chunks = chunks;      // takes effect at the next dfft_init (the pipeline of an initialised plan is not rebuilt:
                                 // dfft_get_pipeline_chunks keeps reporting the depth in use until then)
    return 0;
}
int dfft_get_pipeline_chunks(const dfft_plan *p) { return p ? p->pl.C : 0; }

int dfft_set_stream(dfft_plan *p, void *hip_stream)
{
    if (!p) return fail(ERR_ARG, "null plan");
    graphs_clear(p);
    if (p->stream_owned && p->stream) (void)hipStreamDestroy(p->stream);
    p->stream = (hipStream_t)hip_stream;
    p->stream_owned = false;
    p->stream_user = true;
    return 0;
}

int dfft_enqueue_c2c(dfft_plan *p, void *out, void *in, int direction)
{
    TRY(check_ready(p));
    if (!p->c2c) return fail(ERR_STATE, "plan was initialised for R2C/C2R");
    if (!out || !in) return fail(ERR_ARG, "null buffer");
    if (direction == DFFT_FORWARD || direction == DFFT_INVERSE)
        return run_graphed(p, direction == DFFT_INVERSE, in, out, [&]() { return run_chain(p, direction, 3, out, in); });
    return fail(ERR_ARG, "direction must be DFFT_FORWARD or DFFT_INVERSE");
}

int dfft_exec_c2c(dfft_plan *p, void *out, void *in, int direction)
{
    TRY(dfft_enqueue_c2c(p, out, in, direction));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}

int dfft_exec_dim(dfft_plan *p, void *out, void *in, int direction, int d)
{
    TRY(check_ready(p));
    if (!out || !in) return fail(ERR_ARG, "null buffer");
    if (d < 1 || d > 3) return fail(ERR_ARG, "d must be 1, 2 or 3");
    if (direction != DFFT_FORWARD && direction != DFFT_INVERSE) return fail(ERR_ARG, "bad direction");
    if ((p->zyx || p->yzx) && d != 3) return fail(ERR_UNSUPPORTED, "partial transforms are not defined for the Z_Then_YX / Y_Then_ZX sequences");
    const int kind = 2 * d + (direction == DFFT_INVERSE ? 1 : 0) + 8;
    TRY(run_graphed(p, kind, in, out, [&]() { return run_chain(p, direction, d, out, in); }));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}

int dfft_exchange(dfft_plan *p, int which, int direction, const void *sendbuf, void *recvbuf)
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    if (which != 1 && which != 2) return fail(ERR_ARG, "which must be 1 or 2");
    // host-only callers (callback transport on a machine without a GPU) have no stream to drain; with a
    // device the exchange always runs on a stream of the plan and is complete on return
    int ndev = 0;
    const bool gpu = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    if (gpu && !p->stream && !p->stream_user) {
        HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
        p->stream_owned = true;
    }
    if ((which == 1 ? p->P2 : p->P1) > 1) TRY(exchange(p, which, direction != DFFT_INVERSE, sendbuf, recvbuf));
    if (gpu) HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}

int dfft_exec_r2c(dfft_plan *p, void *out, const void *in)
{
    TRY(check_ready(p));
    if (p->c2c) return fail(ERR_STATE, "plan was initialised for C2C");
    if (!out || !in) return fail(ERR_ARG, "null buffer");
    TRY(run_graphed(p, 2, in, out, [&]() { return run_chain(p, DFFT_FORWARD, 3, out, in); }));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}
int dfft_exec_c2r(dfft_plan *p, void *out, void *in)
{
    TRY(check_ready(p));
    if (p->c2c) return fail(ERR_STATE, "plan was initialised for C2C");
    if (!out || !in) return fail(ERR_ARG, "null buffer");
    TRY(run_graphed(p, 3, in, out, [&]() { return run_chain(p, DFFT_INVERSE, 3, out, in); }));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}

int dfft_spectral_op_supported(int precision, size_t Nx, int option_value)
{
    if ((precision != DFFT_F64 && precision != DFFT_F32) || (option_value != 1 && option_value != 2)) return 0;
    Axis ax;
    if (!axis_plan(precision, Nx, ax)) return 0;      // the x axis of dfft_init with default options
    return spectral_kernel_for(precision, ax, option_value, nullptr) != SPECTRAL_NONE ? 1 : 0;
}

// The operator of a spectral-operator exec: checks `op` (`which`: "" or the " ops[j]" the message names) and copies the fields its
// kind reads into `dst`.  One function for dfft_exec_spectral_op and every operator of dfft_exec_spectral_ops
static int take_spectral_op(const dfft_plan *p, const dfft_spectral_op *op, const std::string &which, dfft_spectral_op &dst)
{
    const std::string pre = "spectral_op" + which + ": ";
    if (op->kind < 0 || op->kind > 5)
        return fail(ERR_ARG, pre + "kind must be 0 (array), 1 (sum of tables), 2 (reciprocal of the sum), 3 (product of factor tables), "
                                   "4 (product times the sum) or 5 (product over the sum)");
    // the fields a kind does not use are never read: cx, cy, cz were appended, a caller of kinds 0 .. 2 may hold the six-field struct
    const bool sums = op->kind == 1 || op->kind == 2 || op->kind == 4 || op->kind == 5, factors = op->kind >= 3;
    if (op->kind == 0 && !op->mult) return fail(ERR_ARG, pre + "null multiplier");
    if (sums && (!op->ax || !op->ay || !op->az)) return fail(ERR_ARG, pre + "null multiplier (kinds 1, 2, 4 and 5 need all of ax, ay, az)");
    if (factors && !op->cx && !op->cy && !op->cz) return fail(ERR_ARG, pre + "null multiplier (kinds 3, 4 and 5 need at least one of cx, cy, cz)");
    if (op->kind == 0) {
        // one tile per workgroup: the kernel adds 32-bit lane offsets (t*MK + l*ME elements) to a scalar base per point.  G and the threads
        // per line are the axis pass's: a configuration of the fused kernel's own (spectral_mixed.inc) has the same G and, at G = 1, no more
        // threads per line (asserted in spectral_mixed.hip.inc), so the bound holds for it too
        PassInfo pi;
        const Launch *L = p->pl.groups[G_XX].L.empty() ? nullptr : &p->pl.groups[G_XX].L[0];
        if (L && pass_info(p->prec, (int)p->Nx, &pi) && pi.G == 1 &&
            ((uint64_t)(pi.N / pi.E) * L->args.MK + (uint64_t)pi.TL * L->args.ME) * p->esz >= (1ull << 32))
            return fail(ERR_UNSUPPORTED, pre + "the multiplier block is too large for the kernel's 32-bit lane offsets");
    }
    dst = dfft_spectral_op{};
    dst.kind = op->kind; dst.scale = op->scale;
    if (op->kind == 0) dst.mult = op->mult;
    if (sums) { dst.ax = op->ax; dst.ay = op->ay; dst.az = op->az; }
    if (factors) { dst.cx = op->cx; dst.cy = op->cy; dst.cz = op->cz; }
    return 0;
}

int dfft_exec_spectral_op(dfft_plan *p, void *out, const void *in, const dfft_spectral_op *op)
{
    if (p && p->initialized && p->pl.spec.steps.empty())
        return fail(ERR_STATE, "plan was initialised without option spectral_op (set it before dfft_init)");
    TRY(check_ready(p));
    if (!out || !in || !op) return fail(ERR_ARG, "null buffer or operator");
    if (out == in) return fail(ERR_ARG, "spectral_op: out == in is not supported");
    TRY(take_spectral_op(p, op, "", p->ops[0]));
    TRY(run_chain(p, DFFT_SPECTRAL_OP, 3, out, in));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}

int dfft_exec_spectral_ops(dfft_plan *p, int nout, void *const *outs, const void *in, const dfft_spectral_op *ops)
{
    if (p && p->initialized && p->pl.spec_multi.steps.empty()) return fail(ERR_STATE, "set spectral_outputs before dfft_init");
    TRY(check_ready(p));
    if (nout < 1 || nout > p->opt.spectral_outputs)
        return fail(ERR_ARG, "spectral_ops: nout must be 1 to " + std::to_string(p->opt.spectral_outputs) + " (option spectral_outputs)");
    if (!outs || !in || !ops) return fail(ERR_ARG, "null buffer or operator");
    for (int j = 0; j < nout; j++) {
        if (!outs[j]) return fail(ERR_ARG, "null buffer or operator");
        if (outs[j] == in) return fail(ERR_ARG, "spectral_ops: outs[" + std::to_string(j) + "] == in is not supported");
        for (int i = 0; i < j; i++)
            if (outs[i] == outs[j]) return fail(ERR_ARG, "spectral_ops: outs[" + std::to_string(i) + "] == outs[" + std::to_string(j) + "]");
    }
    for (int j = 0; j < nout; j++) {
        TRY(take_spectral_op(p, &ops[j], " ops[" + std::to_string(j) + "]", p->ops[j]));
        p->outs[j] = outs[j];
    }
    // the slices do not depend on the number of outputs: fewer of them are the first steps of the plan's chain
    Chain ch = p->pl.spec_multi;
    ch.steps.resize((size_t)(2 + 3 * nout));
    TRY(run_chain(p, DFFT_SPECTRAL_OPS, 3, outs[0], in, &ch));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}

int dfft_exec_spectral_sum(dfft_plan *p, void *out, int nin, const void *const *ins, const dfft_spectral_op *ops)
{
    if (p && p->initialized && p->pl.spec_sum.steps.empty()) return fail(ERR_STATE, "set spectral_inputs before dfft_init");
    TRY(check_ready(p));
    if (nin < 1 || nin > p->opt.spectral_inputs)
        return fail(ERR_ARG, "spectral_sum: nin must be 1 to " + std::to_string(p->opt.spectral_inputs) + " (option spectral_inputs)");
    if (!out || !ins || !ops) return fail(ERR_ARG, "null buffer or operator");
    for (int j = 0; j < nin; j++) {
        if (!ins[j]) return fail(ERR_ARG, "null buffer or operator");
        if (ins[j] == out) return fail(ERR_ARG, "spectral_sum: out == ins[" + std::to_string(j) + "] is not supported");
    }
    dfft_spectral_op taken[DFFT_SPECTRAL_MAX_INPUTS];
    for (int j = 0; j < nin; j++) {
        const std::string which = " ops[" + std::to_string(j) + "]";
        TRY(take_spectral_op(p, &ops[j], which, taken[j]));
        // K domain-sized multiplier arrays, the 11-trip form: the accumulating kernels exist for the table forms alone
        if (taken[j].kind == 0)
            return fail(ERR_UNSUPPORTED, "spectral_op" + which + ": kind 0 (array) is not supported, the sum takes the table forms, kinds 1-5");
    }
    for (int j = 0; j < nin; j++) { p->ops[j] = taken[j]; p->ins[j] = ins[j]; }
    // exchange 2 backwards follows the last xx, so fewer inputs are not a prefix of the plan's chain; the slices do not depend on nin
    const Chain ch = nin == p->opt.spectral_inputs ? p->pl.spec_sum : spectral_sum_chain(p, nin);
    TRY(run_chain(p, DFFT_SPECTRAL_SUM, 3, out, ins[0], &ch));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}

int dfft_get_in_size(const dfft_plan *p, size_t s[3])
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    s[0] = p->xs[p->pi]; s[1] = p->ys[p->pj]; s[2] = p->Nz;
    return 0;
}
int dfft_get_in_start(const dfft_plan *p, size_t s[3])
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    s[0] = p->xstart[p->pi]; s[1] = p->ystart[p->pj]; s[2] = 0;
    return 0;
}
int dfft_get_out_size(const dfft_plan *p, size_t s[3])
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    s[0] = p->Nx; s[1] = p->yo[p->pi]; s[2] = p->zs[p->pj];
    if (p->zyx) { s[1] = p->Ny; s[2] = p->zs[p->pi]; }      // include/mpicufft_slab_z_then_yx.hpp:43-44
    return 0;
}
int dfft_get_out_start(const dfft_plan *p, size_t s[3])
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    s[0] = 0; s[1] = p->yostart[p->pi]; s[2] = p->zstart[p->pj];
    if (p->zyx) { s[1] = 0; s[2] = p->zstart[p->pi]; }
    return 0;
}
int dfft_get_out_strides(const dfft_plan *p, size_t s[3])
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    size_t n[3];
    (void)dfft_get_out_size(p, n);
    if (p->opt.spectral) { s[0] = 1; s[1] = n[2] * n[0]; s[2] = n[0]; }      // [yo][zs][Nx]
    else { s[0] = n[1] * n[2]; s[1] = n[2]; s[2] = 1; }                       // [Nx][yo][zs] (and the slab sequences' [Nx][Ny][zs], [Nx][yo][Nz])
    return 0;
}
int dfft_get_partition_dimensions(const dfft_plan *p, int which, int axis, size_t *sizes, size_t *starts, size_t capacity,
                                  size_t *count)
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    if (which < 0 || which > 2 || axis < 0 || axis > 2) return fail(ERR_ARG, "which and axis must be 0, 1 or 2");
    // input_dim / transposed_dim / output_dim of src/pencil/mpicufft_pencil_opt1.cpp:70-93; an axis that is not
    // split at that stage has one entry holding its full extent
    const std::vector<size_t> one_x{p->Nx}, one_y{which == 2 ? p->Nyc : p->Ny}, one_z{which == 0 ? p->Nz : p->Nzc}, zero{0};
    const std::vector<size_t> *sz = nullptr, *st = &zero;
    if (axis == 0) {
        if (which == 2) sz = &one_x; else { sz = &p->xs; st = &p->xstart; }
    } else if (axis == 1) {
        if (which == 0) { sz = &p->ys; st = &p->ystart; }
        else if (which == 1 || p->zyx) sz = &one_y;
        else { sz = &p->yo; st = &p->yostart; }
    } else {
        if (which == 0 || p->yzx) sz = &one_z; else { sz = &p->zs; st = &p->zstart; }
    }
    if (count) *count = sz->size();
    for (size_t i = 0; i < sz->size() && i < capacity; i++) {
        if (sizes) sizes[i] = (*sz)[i];
        if (starts) starts[i] = st->size() == sz->size() ? (*st)[i] : 0;
    }
    return 0;
}
size_t dfft_domain_size(const dfft_plan *p) { return p ? p->domainsize : 0; }
size_t dfft_work_size_device(const dfft_plan *p) { return p ? p->worksize_d : 0; }
size_t dfft_work_size_host(const dfft_plan *p) { (void)p; return 0; }
void *dfft_work_area_device(const dfft_plan *p) { return p ? p->work_d : nullptr; }
int dfft_rank(const dfft_plan *p) { return p ? p->rank : -1; }
int dfft_world_size(const dfft_plan *p) { return p ? p->nranks : 0; }
int dfft_tile_lines(const dfft_plan *p) { return p ? p->TL : 0; }

int dfft_get_exchange_tables(const dfft_plan *p, int which, size_t *sc, size_t *sd, size_t *rc, size_t *rd)
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    if (which != 1 && which != 2) return fail(ERR_ARG, "which must be 1 or 2");
    const auto &a = which == 1 ? p->sc1 : p->sc2, &b = which == 1 ? p->sd1 : p->sd2;
    const auto &c = which == 1 ? p->rc1 : p->rc2, &d = which == 1 ? p->rd1 : p->rd2;
    for (size_t i = 0; i < a.size(); i++) { sc[i] = a[i]; sd[i] = b[i]; rc[i] = c[i]; rd[i] = d[i]; }
    return 0;
}

int dfft_get_pipeline_tables(const dfft_plan *p, int direction, int which, int chunk, size_t *sc, size_t *sd,
                             size_t *rc, size_t *rd)
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    if (which != 1 && which != 2) return fail(ERR_ARG, "which must be 1 or 2");
    if (chunk < 0 || chunk >= p->pl.C) return fail(ERR_ARG, "chunk out of range");
    const std::vector<A2A> &v = direction == DFFT_INVERSE ? (which == 1 ? p->pl.i1 : p->pl.i2)
                                                          : (which == 1 ? p->pl.f1 : p->pl.f2);
    if ((size_t)chunk >= v.size()) return fail(ERR_ARG, "this plan has no such exchange");
    const A2A &T = v[chunk];
    for (size_t i = 0; i < T.sc.size(); i++) { sc[i] = T.sc[i]; sd[i] = T.sd[i]; rc[i] = T.rc[i]; rd[i] = T.rd[i]; }
    return 0;
}

static const Launch *find_launch(const dfft_plan *p, const char *name, int index)
{
    for (const Group &g : p->pl.groups)
        if (name && !strcmp(g.name, name)) return index >= 0 && (size_t)index < g.L.size() ? &g.L[(size_t)index] : nullptr;
    return nullptr;
}

int dfft_debug_get_pass(const dfft_plan *p, const char *name, int index, dfft_pass_desc *d)
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    if (!d) return fail(ERR_ARG, "null descriptor");
    const Launch *L = find_launch(p, name, index);
    if (!L) return fail(ERR_ARG, "the plan has no such launch");
    const PassArgs &A = L->args;
    memset(d, 0, sizeof(*d));
    d->na = A.na; d->LB = A.LB; d->nb = A.nb; d->LA = A.LA; d->T2shift = A.T2shift;
    d->load_kind = A.load_kind; d->store_kind = A.store_kind; d->swap = A.swap; d->shift = A.shift;
    d->KS_in = A.KS_in; d->KS_out = A.KS_out; d->AS_in = A.AS_in; d->AS_out = A.AS_out;
    d->IA = A.IA; d->IB = A.IB; d->SK = A.SK; d->SB = A.SB; d->a_fastest = A.a_fastest; d->xcd_swizzle = A.xcd_swizzle;
    d->in_off = L->in_off; d->out_off = L->out_off;
    d->lnseg = L->lseg.nseg; d->snseg = L->sseg.nseg;
    for (int s = 0; s < L->lseg.nseg; s++) { d->lstart[s] = L->lseg.start[s]; d->llen[s] = L->lseg.len[s]; d->lbase[s] = L->lseg.base[s]; }
    for (int s = 0; s < L->sseg.nseg; s++) { d->sstart[s] = L->sseg.start[s]; d->slen[s] = L->sseg.len[s]; d->sbase[s] = L->sseg.base[s]; }
    return 0;
}

int dfft_debug_get_chain(const dfft_plan *p, int direction, int dims, dfft_chain_step *steps, int capacity, int *count)
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    const bool spec = (direction == DFFT_SPECTRAL_OP || direction == DFFT_SPECTRAL_OPS || direction == DFFT_SPECTRAL_SUM) && dims == 3;
    if (dims < 1 || dims > 3 || (direction != DFFT_FORWARD && direction != DFFT_INVERSE && !spec)) return fail(ERR_ARG, "bad direction or dims");
    const Chain &ch = chain_of(p, direction, dims);
    const std::vector<Step> &st = ch.steps;
    if (count) *count = (int)st.size();
    for (size_t i = 0; i < st.size() && (int)i < capacity; i++) {
        const Step &s = st[i];
        const Group &g = p->pl.groups[s.group];
        dfft_chain_step &d = steps[i];
        memset(&d, 0, sizeof(d));
        strncpy(d.group, g.name, sizeof(d.group) - 1);
        d.axis = g.axis; d.launches = (int32_t)g.L.size(); d.per_chunk = s.per_chunk;
        d.src = s.src; d.dst = s.dst; d.conj = s.conj; d.form = s.form; d.exchange = s.xchg; d.split = ch.split;
        d.tables = s.tables ? s.tables : (direction == DFFT_INVERSE ? DFFT_INVERSE : DFFT_FORWARD);
    }
    return 0;
}

int dfft_debug_trace_chain(const dfft_plan *p, int direction, int dims, dfft_trace_op *ops, int capacity, int *count)
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    const bool spec = (direction == DFFT_SPECTRAL_OP || direction == DFFT_SPECTRAL_OPS || direction == DFFT_SPECTRAL_SUM) && (dims == 3 || dims == 0);
    if (dims < 0 || dims > 3 || (direction != DFFT_FORWARD && direction != DFFT_INVERSE && !spec)) return fail(ERR_ARG, "bad direction or dims");
    std::vector<dfft_trace_op> dry;
    if (dims > 0) {
        const Chain &ch = chain_of(p, direction, dims);
        DrySink sk{p, ch.steps, dry};
        TRY(schedule_chain(p, ch, streams_of(p, ch), sk));
    }
    const std::vector<dfft_trace_op> &v = dims > 0 ? dry : p->trace_log[trace_slot(direction)];
    if (count) *count = (int)v.size();
    for (size_t i = 0; i < v.size() && (int)i < capacity; i++) ops[i] = v[i];
    return 0;
}

int dfft_get_pass_choices(const dfft_plan *p, int variant[6], int order[6], int addr64[6])
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    for (int k = 0; k < 6; k++) {
        const std::vector<Launch> *v = pass_launches(const_cast<dfft_plan *>(p), k);
        const Launch *L = v && !v->empty() ? &(*v)[0] : nullptr;
        if (variant) variant[k] = k < 3 ? p->vfwd[k] : p->vinv[5 - k];
        if (order) order[k] = L ? (L->args.a_fastest ? 1 : 0) + (L->args.xcd_swizzle ? 2 : 0) : -1;
        if (addr64) addr64[k] = L ? L->args.addr64 : -1;
    }
    return 0;
}

int dfft_debug_get_point_table(const dfft_plan *p, const char *name, int index, int store, uint64_t *base, uint32_t *ln,
                               uint32_t *aux, size_t capacity, size_t *count)
{
    if (!p || !p->initialized) return fail(ERR_STATE, "plan not initialised");
    const Launch *L = find_launch(p, name, index);
    if (!L) return fail(ERR_ARG, "the plan has no such launch");
    const SegTable &T = store ? L->sseg : L->lseg;
    const bool tiled = store ? (L->args.store_kind == STORE_TILED_SAME || L->args.store_kind == STORE_TILED_TRANSPOSE)
                             : L->args.load_kind == LOAD_TILED;
    if (!tiled || T.nseg < 1) return fail(ERR_ARG, "that side of the launch is not segmented");
    std::vector<SegEntry> tab;
    point_table(*L, store != 0, tab);
    if (count) *count = tab.size();
    for (size_t i = 0; i < tab.size() && i < capacity; i++) {
        if (base) base[i] = tab[i].base;
        if (ln) ln[i] = tab[i].ln;
        if (aux) aux[i] = tab[i].aux;
    }
    return 0;
}

int dfft_enable_phase_timing(dfft_plan *p, int enable)
{
    if (!p) return fail(ERR_ARG, "null plan");
    p->timing = enable != 0;
    graphs_clear(p);
    return 0;
}
int dfft_get_phase_times(dfft_plan *p, float *ms, int max_entries)
{
    if (!p) return fail(ERR_ARG, "null plan");
    // sums per phase over all chunks: 0 first FFT pass, 1 first exchange, 2 second pass,
    // 3 second exchange, 4 last pass (overlapping spans are both counted in full)
    float acc[5] = {0, 0, 0, 0, 0};
    for (size_t i = 0; i < p->nspans; i++) {
        float t = 0;
        if (hipEventElapsedTime(&t, p->spans[i].a, p->spans[i].b) == hipSuccess) acc[p->spans[i].phase] += t;
    }
    int n = 0;
    for (; n < 5 && n < max_entries; n++) ms[n] = acc[n];
    return p->nspans ? n : 0;
}
const char *dfft_phase_name(int phase, int direction)
{
    static const char *f[] = {"z-FFT", "exchange 1", "y-FFT", "exchange 2", "x-FFT"};
    static const char *b[] = {"x-FFT^-1", "exchange 2", "y-FFT^-1", "exchange 1", "z-FFT^-1"};
    if (phase < 0 || phase > 4) return "";
    return direction == DFFT_INVERSE ? b[phase] : f[phase];
}

int dfft_fft1d_batched_ex(int precision, size_t N, size_t batch, void *out, const void *in, int direction,
                          void *hip_stream, int variant, int debug)
{
    static thread_local Axis ax;
    static thread_local int axP = -1;
    static thread_local int axB = 0;
    // scratch of two-level lines, grown on demand, one per stream: two calls of one thread on different streams must not share it
    // (growing it frees the old one with hipFree, which waits for every launch still using it)
    static thread_local std::map<void *, std::pair<void *, size_t>> lvw_of;
    // bounded: a thread that keeps calling on fresh streams (streams come and go) must not pile up scratch buffers -- beyond 8
    // entries everything but this stream's is released (hipFree waits for the launches that still use it)
    if (lvw_of.size() > 8 && !lvw_of.count(hip_stream)) {
        for (auto &kv : lvw_of) if (kv.second.first) (void)hipFree(kv.second.first);
        lvw_of.clear();
    }
    void *&lvw = lvw_of[hip_stream].first;
    size_t &lvw_bytes = lvw_of[hip_stream].second;
    // variant -1: the Bluestein kernel even where a native configuration exists; -2: two levels wherever the length splits
    const int force = variant == -2 ? 2 : variant < 0 ? 1 : 0;
    if (variant > 15) return fail(ERR_ARG, "variant must be -2 (two-level), -1 (Bluestein) or 0..15");
    if (force) variant = 0;
    if (ax.N != N || axP != precision || axB != force) {
        axis_free(ax);
        ax = Axis();
        axP = -1;
        if (!(force == 1 ? axis_plan_bluestein(precision, N, ax) : axis_plan(precision, N, ax, true, force == 2))) { ax = Axis(); return fail(ERR_UNSUPPORTED, "unsupported line length"); }
        std::string why;
        if ((ax.bluestein || !is_pow2(ax.N)) && !any_available(&why)) { ax = Axis(); return fail(ERR_UNSUPPORTED, "this line length needs the kernels of libdfft_amd_any.so: " + why); }
        if (int r = axis_upload(precision, ax)) { axis_free(ax); ax = Axis(); return r; }
        axP = precision;
        axB = force;
    }
#ifdef DFFT_EXPERIMENTS
    if ((variant == 15 || variant == 14) && precision == DFFT_F32 && !ax.bluestein) {      // A/B: the LDS-free shuffle pass (15 bpermute, 14 DPP)
        PassArgs S;
        memset(&S, 0, sizeof(S));
        S.in = in; S.out = out; S.tw = ax.tw; S.na = 1; S.LB = (uint32_t)batch; S.swap = direction == DFFT_INVERSE;
        const int r = launch_shfl_f32((int)N, variant == 14, S, (hipStream_t)hip_stream);
        return r == 0 ? 0 : fail(r == -1 ? ERR_UNSUPPORTED : r, "shuffle pass launch failed");
    }
#endif
    PassInfo pi;      // the tile lines of the configuration that runs: the variant's, else the default one's
    if (!(variant && has_variant(precision, ax, variant, &pi))) {
        variant = 0;
        if (!pass_info(precision, ax.two || ax.longb ? 2 : (int)ax.M, &pi)) return fail(ERR_UNSUPPORTED, "unsupported line length");      // (two levels: any configuration gives TL)
    }
    PassArgs A;
    memset(&A, 0, sizeof(A));
    A.in = in; A.out = out; A.tw = ax.tw; A.debug = debug;
    A.na = 1; A.LB = (uint32_t)batch; A.nb = ((uint32_t)batch + pi.TL - 1) / pi.TL; A.ntiles = A.nb;
    A.load_kind = LOAD_LINES; A.store_kind = STORE_LINES; A.swap = direction == DFFT_INVERSE;
    const size_t need = axis_scratch_bytes(precision, ax, A, pi.TL);
    if (need > lvw_bytes) {
        if (lvw) { (void)hipFree(lvw); lvw = nullptr; lvw_bytes = 0; }      // (hipFree waits for the launches that still use it)
        HIP_TRY(hipMalloc(&lvw, need));
        lvw_bytes = need;
    }
    return launch_axis(precision, ax, A, variant, 0, N, lvw, lvw_bytes, pi.TL, (hipStream_t)hip_stream);
}
int dfft_fft1d_batched(int precision, size_t N, size_t batch, void *out, const void *in, int direction,
                       void *hip_stream)
{
    return dfft_fft1d_batched_ex(precision, N, batch, out, in, direction, hip_stream, 0, 0);
}

int dfft_kernel_info(int precision, size_t N, int *threads, int *lds_bytes, int *points_per_thread,
                     int *lines_per_workgroup)
{
    PassInfo pi;
    Axis a;
    if (!axis_plan(precision, N, a) || !pass_info(precision, (int)(a.longb ? a.lv[0].lv[1].M : a.two ? a.lv[1].M : a.M), &pi)) return ERR_UNSUPPORTED;      // two levels: the second level's kernel
    if (threads) *threads = pi.threads;
    if (lds_bytes) *lds_bytes = pi.lds_bytes;
    if (points_per_thread) *points_per_thread = pi.E;
    if (lines_per_workgroup) *lines_per_workgroup = pi.TL * pi.G / (pi.sub > 1 ? pi.sub : 1);      // sub-tile workgroups: part of a tile
    return 0;
}

int dfft_axis_plan_info(int precision, size_t N, int two_level, size_t info[8])
{
    if (!info) return fail(ERR_ARG, "null pointer");
    Axis a;
    if (!axis_plan(precision, N, a, true, two_level)) return ERR_UNSUPPORTED;
    for (int k = 0; k < 8; k++) info[k] = 0;
    info[0] = a.longb ? 3 : a.two ? 2 : a.bluestein ? 1 : 0;
    info[1] = a.M;
    if (a.longb) a = Axis(a.lv[0]);      // the levels of the padded length
    for (size_t k = 0; k < a.lv.size(); k++) { info[2 + 3 * k] = a.lv[k].N; info[3 + 3 * k] = a.lv[k].M; info[4 + 3 * k] = a.lv[k].bluestein; }
    return 0;
}

int dfft_malloc(size_t bytes, size_t chunk_mib, void **ptr)
{
    if (!ptr) return fail(ERR_ARG, "null pointer");
    if (chunk_mib == DFFT_CHUNK_DEFAULT) return dev_alloc_default(bytes, ptr);
    return dev_alloc(bytes, chunk_mib, ptr);
}
int dfft_free(void *ptr) { return dev_free(ptr); }
int dfft_last_placement_info(char *buf, size_t capacity)
{
    if (!buf || !capacity) return fail(ERR_ARG, "null buffer");
    return placement_info_json(buf, capacity);
}

}  // extern "C"
