// plan.hpp -- the plan object of libdfft_amd.so and what its host translation units share: dfft.hip (dfft_init, execution chains,
// C ABI), axis.hip (axis plans and their launches: axis.hpp), pipeline.hip (the pass descriptors and exchange tables of every
// decomposition) and tune.hip (the tuners).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/dfft_c.h"
#include "comm.hpp"
#include "dfft_internal.hpp"
#include "fft_pass.hip.h"

namespace dfft {

// remainder to the lowest ranks (mpicufft_pencil_opt1.cpp:71-73)
inline void split(size_t n, int p, std::vector<size_t> &size, std::vector<size_t> &start)
{
    size.assign(p, n / p);
    start.assign(p, 0);
    for (size_t i = 0; i < n % p; i++) size[i]++;
    size_t off = 0;
    for (int i = 0; i < p; i++) { start[i] = off; off += size[i]; }
}

inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
inline size_t next_pow2(size_t n) { size_t m = 1; while (m < n) m <<= 1; return m; }

// One axis of the 3-D transform: native Stockham chain, Bluestein on top of it, or two levels of either (N = N1*N2)
struct Axis {
    size_t N = 0;          // line length
    bool bluestein = false;    // the generic kernel (fft_bluestein_kernel) runs the pass: Bluestein, or the levels of a two-level line
    size_t M = 0;          // inner power-of-two length (== N when native)
    void *tw = nullptr;    // exp(-2 pi i j / M), M entries
    void *chirp = nullptr; // Bluestein: exp(-i pi n^2 / N), N entries
    void *bhat = nullptr;  // Bluestein: FFT_M(conj chirp, wrapped) / M
    // two-level line (fft_pass.hip.h, "Two-level lines"): lv[0] transforms N1 = lv[0].N points, lv[1] N2 = lv[1].N; a level is
    // the plain power-of-two chain (bluestein == false, M == N) or Bluestein on an arbitrary factor
    bool two = false;
    // long Bluestein line (a length that neither fits one launch nor splits into two such factors: a prime above 4096, twice such a
    // prime ...): Bluestein's algorithm whose M-point transforms are two-level lines; lv[0] is that two-level plan of M, chirp / bhat as
    // for the one-launch form.  Four launches of the generic kernel (launch_long_bluestein).
    bool longb = false;
    std::vector<Axis> lv;
    void *twN = nullptr;   // exp(-2 pi i j / N), N entries: twiddles between the levels
};

}  // namespace dfft

struct Launch {
    dfft::PassArgs args{};          // in/out/tw and the device table pointers are filled at enqueue time (zeroed: a plan builds only the launches of its kind)
    dfft::SegTable lseg{}, sseg{};  // host copies of the segment tables (uploaded by upload_tables)
    size_t ltab = 0, stab = 0;   // byte offsets of the tables in the plan's device table buffer
    size_t lent = SIZE_MAX, sent = SIZE_MAX;   // byte offsets of the per-point address tables (SIZE_MAX: none)
    size_t in_off = 0;        // byte offset added to the stage's input buffer
    size_t out_off = 0;       // byte offset added to the stage's output buffer
    size_t mult_off = 0;      // xx launches: element offset of the chunk's first ky row in the multiplier array ...
    size_t ty_off = 0;        // ... and in the ky table (dfft_spectral_op)
};
struct A2A {
    std::vector<size_t> sc, sd, rc, rd;   // bytes, absolute displacements in the stage buffers
};

// The launch groups of a plan, one table (Pipeline::groups) under the names dfft_debug_get_pass takes.  G_FZ .. G_IZ are the
// tunable passes 0 .. 5 (fz fy fx ix iy iz: options variant_* / order_*, dfft_get_pass_choices, dfft_tune_variants).
enum GroupId {
    G_FZ, G_FY, G_FX, G_IX, G_IY, G_IZ,   // default sequence (pencil, slab ZY_Then_X): forward z, y (per chunk), x; inverse x, y, z (per chunk)
    G_PZ1, G_QZ1, G_PY2, G_QY2,           // partial transforms (reference: execR2C/C2R(out, in, d), src/pencil/mpicufft_pencil.cpp:1644-1839):
                                          // d = 1 z pass natural -> natural [xs][ys][Nzc] and back; d = 2 y pass chunk -> [xs][Ny][zs] and back
    G_ZY, G_ZIY, G_ZIX,                   // slab sequence Z_Then_YX (src/slab/z_then_yx/): y passes per (chunk, source peer) block, unchunked
                                          // inverse x pass (z passes: fz / iz, forward x pass: fx)
    G_YZ,                                 // Y_Then_ZX: final z pass (x pass = fx, y chunks = fy)
    G_SZ, G_SX, G_SY,                     // single-rank complex plans, pass order z, x, y (build_pipeline_single): natural -> L1 -> L2 -> natural
    G_XX,                                 // option spectral_op: forward x pass, pointwise multiplier and inverse x pass in one launch per ky chunk
                                          // (fft_spectral_kernel): the load side of fx restricted to the chunk's ky rows, the store side of ix[c]
    NGROUPS
};
struct Group {
    const char *name;
    int axis;                  // 0 = z, 1 = y, 2 = x
    std::vector<Launch> L;     // per chunk (zy / ziy: per chunk and peer); empty where the plan has no such launch
};

// One step of an execution chain: the launches of a group, chunk by chunk, with the exchange after each chunk (run_chain, dfft.hip).
enum Buffer { BUF_IN = -2, BUF_OUT = -1 };     // and k >= 0: work-area slice k; -(2 + j): output j >= 1 of a multi-output chain;
                                               // -(9 + j): input j >= 1 of a multi-input chain
inline int buf_output(int j) { return j == 0 ? BUF_OUT : -(2 + j); }
inline int buf_input(int j) { return j == 0 ? BUF_IN : -(9 + j); }
static_assert(-(2 + (DFFT_SPECTRAL_MAX_OUTPUTS - 1)) > -(9 + 1), "the codes of the outputs end above those of the inputs");
// the output a step of a spectral-operator chain belongs to (Pipeline::spec: always 0; spec_multi: by position)
inline int spectral_output_of(int step) { return step < 2 ? 0 : (step - 2) / 3; }
// ... and the input a step of the multi-input chain belongs to (Pipeline::spec_sum: the triples fz, fy, xx come first)
inline int spectral_input_of(int step) { return step / 3; }
enum LineForm {
    FORM_FWD,         // complex lines, kernel configuration vfwd[axis]
    FORM_INV,         // complex lines, vinv[axis]
    FORM_FIXED,       // complex lines, configuration 0
    FORM_REAL_Z1,     // real z pass, mode 1 (R2C)
    FORM_REAL_Z2,     // real z pass, mode 2 (C2R)
    FORM_REAL_LINES,  // real strided lines in, Hermitian half out (the y pass of a Y_Then_ZX R2C plan)
    FORM_FIXED_ACC    // FORM_FIXED, the result added to what dst holds (group xx of the multi-input chain: PassArgs::acc)
};
struct Step {
    int group;             // GroupId (an index: dfft_init may rebuild the launches)
    int form;              // LineForm
    int src, dst;          // Buffer or work slice
    int phase = -1;        // phase-timing slot of its launches (of its exchange: phase + 1); -1 none
    int xchg = 0;          // 1 / 2: that exchange after each chunk, dst -> the next step's src (tables f1 / f2, or i1 / i2 in an inverse chain)
    bool whole = false;    // chunk c waits for the whole step before it (else for chunk c of it only)
    int per_chunk = 1;     // launches per chunk
    bool conj = false;     // launched with conjugation (swap = 1)
    int tables = 0;        // direction whose exchange tables `xchg` uses: DFFT_FORWARD f1 / f2, DFFT_INVERSE i1 / i2; 0 = the chain's own
                           // direction (the spectral-operator chain runs forward exchanges before its xx step and inverse ones after)
};
struct Chain {
    std::vector<Step> steps;
    bool split = false;    // its chunks may alternate over two compute streams (option compute_streams)
};

struct Pipeline {
    int C = 1;
    Group groups[NGROUPS] = {{"fz", 0}, {"fy", 1}, {"fx", 2}, {"ix", 2}, {"iy", 1}, {"iz", 0}, {"pz1", 0}, {"qz1", 0}, {"py2", 1},
                             {"qy2", 1}, {"zy", 1}, {"ziy", 1}, {"zix", 2}, {"yz", 0}, {"sz", 0}, {"sx", 2}, {"sy", 1}, {"xx", 2}};
    // execution chains: fwd[d - 1] / inv[d - 1] of dfft_exec_dim (d = 3: the whole transform); one_fwd / one_inv the alternatives of a
    // single rank's complex plan (one_rank_alternative): the z, x, y order, or (one_inv alone) the forward launches with conjugation
    Chain fwd[3], inv[3], one_fwd, one_inv;
    // option spectral_op (dfft_exec_spectral_op): z -> ex1 -> y -> ex2 -> xx -> ex2^-1 -> y^-1 -> ex1^-1 -> z^-1 on work slices alone
    // (`in` is only read, `out` only written by z^-1); empty without the option
    Chain spec;
    // option spectral_outputs = K >= 2 (dfft_exec_spectral_ops): one forward half, K inverse halves -- fz, fy, then K times xx, iy, iz.
    // The step at position 2 + 3 j + {0, 1, 2} belongs to output j (spectral_output_of): its xx runs operator j, its iz writes output
    // j.  The slices do not depend on K, so an exec of nout < K outputs runs the first 2 + 3 nout steps.  Empty when K == 1
    Chain spec_multi;
    // option spectral_inputs = K >= 2 (dfft_exec_spectral_sum): K forward halves, one inverse half -- K times fz, fy, xx, then iy, iz
    // (spectral_sum_chain, pipeline.hip).  The step at position 3 j + {0, 1, 2} belongs to input j (spectral_input_of): its fz reads
    // input j, its xx runs operator j and, for j >= 1, accumulates.  Empty when K == 1
    Chain spec_sum;
    bool single = false;                       // the z, x, y order is built
    size_t single_work_elems = 0;              // size of the padded L2 buffer
    std::vector<A2A> f1, f2, i2, i1;          // per chunk exchange tables
    std::vector<hipEvent_t> ev;               // reusable events
    // streams beside the plan's own.  Which of them an exec uses is decided by streams_of (dfft.hip), never by whether a handle exists:
    // what that predicate asks for and is not there yet is created when an exec first needs it
    hipStream_t comm_stream = nullptr;
    hipStream_t comm_stream2 = nullptr;       // second exchange of a pencil plan (disjoint links: may overlap the first)
    hipStream_t compute_stream2 = nullptr;    // option compute_streams = 2: the odd pipeline chunks of a pass run here (run_chain)
};

struct TimedSpan { hipEvent_t a = nullptr, b = nullptr; int phase = 0; bool used = false; };

// Tuning knobs of a plan (dfft_set_option; a few have environment defaults read once at plan creation).
// Nothing here is read on the execution path.
struct Options {
    int chunks = 0;          // requested pipeline depth (0 = default)
    int mirror = 0;          // single-rank complex inverse in the mirrored (multi-rank) pass order x, y, z
    int tables = 1;          // per-point address tables: 0 never, 1 sides with more than one segment, 2 always
    int uniform_tables = 1;  // sides whose segments all start at multiples of 16 points: table entries through wave-uniform
                             // (scalar) loads, dfft::PassArgs::luni / suni (0: per-lane vector loads, for A/B runs)
    int shift = -1;          // row-aligned tile windows of odd-pitch point-major stores: -1 auto (fp64), 0 off, 2 always
    int debug = 0;           // dfft::PassArgs::debug of every launch (measurement only; results are wrong when set)
    int real_variant = 0;    // A/B configurations of the real z passes (DFFT_EXPERIMENTS builds)
    int single_order = -1;   // single-rank complex plans: 1 = pass order z, x, y with padded private layouts, 0 = z, y, x,
                             // -1 = by measurement: z, x, y where it won (fp32 with x and y lines of 2048 points or more)
    int single_layout = 1;   // L2 of the z, x, y order: 0 = [kx][kz/TL][y][l], 1 = tile-outer [kz/TL][kx][y][l]
    int single_pad = 128;    // bytes added to every L2 row (a row stride that is an odd multiple of 128 B; 0 = packed)
    int graph = 0;           // 1: single-rank plans replay the launches of an exec as one hipGraph from the second call with the same
                             // buffers on.  Off by default -- measured (profiles/r2_graph_latency.txt): a blocking 64^3 R2C takes 28 us
                             // with three plain launches and 34 us as a graph, 128^3 54 vs 60 us; the launches are already hidden
                             // behind the first kernel (128^3: 50 us of kernels in a 54 us call)
    int native_mixed = 1;    // lengths 2^a 3^b 5^c 7^d with a configuration run the native chain (0: Bluestein, for A/B runs and tests)
    int two_level = 0;       // 1: every axis whose length splits as N1*N2 runs as a two-level line (tests, A/B runs; 0: only lengths
                             // that have no other plan)
    int spectral = 0;        // 1: the spectrum is kept x-contiguous, [yo][zs][Nx] (lines along kx natural), instead of the reference's
                             // [Nx][yo][zs]: the forward x pass stores natural lines and the inverse x pass loads them -- neither
                             // touches the point-major layout whose strided read is the slowest pass of every multi-rank plan
    int spectral_op = 0;     // 1 / 2 (2: mixed-radix x lengths as well): the plan also builds the fused forward-multiply-inverse chain (Pipeline::spec, group xx) and one more
                             // work slice for it; 0: nothing of it exists
    int spectral_outputs = 1; // 1 .. 8 (DFFT_SPECTRAL_MAX_OUTPUTS), needs spectral_op: from 2 on the plan also builds Pipeline::spec_multi for
                             // dfft_exec_spectral_ops and, where that chain needs it, one more work slice; 1: nothing of it exists
    int spectral_inputs = 1; // 1 .. 8 (DFFT_SPECTRAL_MAX_INPUTS), needs spectral_op: from 2 on the plan also builds Pipeline::spec_sum for
                             // dfft_exec_spectral_sum and one more work slice, the accumulator (shared with spectral_outputs' extra slice)
    int compute_streams = -1; // 2: the pipeline chunks of a pass alternate over two compute streams, so that the drain of chunk c
                             // overlaps the ramp of chunk c + 1 (a chunk launch of 0.1-0.2 ms pays ~20 us of launch / drain / ramp when
                             // the chunks queue up behind each other on one stream).  -1 = by measurement
                             // (profiles/r6_compute_streams.txt): two streams from three chunks per pass on (rank 0 of 2x4, 1024^3
                             // fp64: 4 chunks 4.89 -> 4.78 ms, 8 chunks 5.31 -> 4.90; at two chunks there is nothing to gain), 1 = one
    int trace = 0;           // debug: 1 = every exec keeps the list of what it issued (dfft_debug_trace_chain with dims = 0)
    int order[6] = {-1, -1, -1, -1, -1, -1};     // workgroup->tile order per pass: fz fy fx ix iy iz; a_fastest + 2*xcd_swizzle
    int variant[6] = {-1, -1, -1, -1, -1, -1};   // kernel configuration per pass, same order (-1 = the plan's choice)
};

struct dfft_plan {
    int kind = DFFT_PENCIL_OPT1, prec = DFFT_F64;
    dfft_config cfg{};
    dfft_comm *comm = nullptr;
    int rank = 0, nranks = 1;
    bool initialized = false, c2c = false;
    bool spectral_mirror = false;   // one rank with an x-contiguous spectrum (option spectral_layout): the inverse runs the mirrored pass order
    bool zyx = false;            // slab sequence Z_Then_YX: input split along x, output split along z
    bool yzx = false;            // slab sequence Y_Then_ZX: R2C along y, output [Nx][(Ny/2+1)/P][Nz], forward only
    size_t Nyc = 0;              // y extent of the spectrum (Ny/2+1 for a Y_Then_ZX R2C plan, else Ny)
    size_t Nx = 0, Ny = 0, Nz = 0, Nzc = 0;
    int P1 = 1, P2 = 1, pi = 0, pj = 0;
    int TL = 8;
    std::vector<size_t> xs, xstart, ys, ystart, zs, zstart, yo, yostart;
    size_t esz = 16, domain_elems = 0, domainsize = 0, worksize_d = 0;
    void *work_d = nullptr;
    bool work_owned = false;
    dfft::Axis ax[3];                  // [0] = z, [1] = y, [2] = x
    bool zreal_native = false;   // R2C plan whose z axis uses the packed Nz/2-point kernels
    bool yreal_native = false;   // Y_Then_ZX R2C plan whose y axis uses the packed Ny/2-point kernel (strided real lines)
    size_t lv_off = 0, lv_bytes = 0;   // two-level axes: scratch between the levels, a region of the work area (behind the exchange slices)
    void *tw_zr = nullptr;       // split/merge table exp(-2 pi i k / Nz) (or / Ny) of the packed real kernels
    void *tables_d = nullptr;    // segment tables of every launch, device copy
    hipStream_t stream = nullptr;
    bool stream_owned = false;
    bool stream_user = false;    // caller chose the stream (the null stream is a valid choice)
    // exchange tables in bytes (row comm = 1, column comm = 2) and member lists
    std::vector<size_t> sc1, sd1, rc1, rd1, sc2, sd2, rc2, rd2;
    std::vector<int> group1, group2;
    dfft::RelayCache *relay = nullptr;      // two-hop relay of the group exchanges (dfft_comm_set_option "relay"): gathered world tables, staging
    int vfwd[3] = {0, 0, 0}, vinv[3] = {0, 0, 0};   // kernel variant per pass: [0]=z [1]=y [2]=x
    Options opt;
    Pipeline pl;
    // phase timing: (start, stop) event pairs, phases 0..4 = z, exchange 1, y, exchange 2, x
    bool timing = false;
    std::vector<TimedSpan> spans;
    size_t nspans = 0;
    int last_dir = -1;
    std::vector<dfft_trace_op> trace_log[5];   // option trace: what the last forward / inverse / spectral-operator / multi-output / multi-input exec issued
    // the spectral-operator exec being enqueued: the multiplier of output j and, for j >= 1, its buffer (output 0 is the exec's `out`)
    // (dfft_exec_spectral_sum: the multiplier of input j and, for j >= 1, its buffer; input 0 is the exec's `in`)
    static_assert(DFFT_SPECTRAL_MAX_INPUTS <= DFFT_SPECTRAL_MAX_OUTPUTS, "ops holds one operator per output or input");
    dfft_spectral_op ops[DFFT_SPECTRAL_MAX_OUTPUTS] = {};
    void *outs[DFFT_SPECTRAL_MAX_OUTPUTS] = {};
    const void *ins[DFFT_SPECTRAL_MAX_INPUTS] = {};
    int spectral_kernel = 0;                   // option spectral_op: the fused x kernel dfft_init found (dfft::SpectralKernel, axis.hpp)
    // hipGraph replay of single-rank execs (launch-bound small grids): one instantiated graph per (operation, in, out)
    struct GraphEntry { int kind; const void *in; void *out; int uses; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs;
};

// pass descriptors and exchange tables of a plan (pipeline.hip): the default sequence (pencil and slab ZY_Then_X), the slab sequences
// Z_Then_YX and Y_Then_ZX, and the single-rank order z, x, y.  Return 0 or an error code (message: dfft_last_error).
int build_pipeline(dfft_plan *p, Pipeline &pl);
int build_pipeline_zyx(dfft_plan *p, Pipeline &pl);
int build_pipeline_yzx(dfft_plan *p, Pipeline &pl);
int build_pipeline_single(dfft_plan *p, Pipeline &pl);
// the multi-input spectral chain for nin inputs (option spectral_inputs; the slices do not depend on nin)
Chain spectral_sum_chain(const dfft_plan *p, int nin);
// shared by dfft.hip and tune.hip
int check_ready(dfft_plan *p);       // 0 when the plan is initialised and has its device state, else an error code
// a single rank's complex plan may run its one-rank alternative chains (neither mirror_inverse nor an x-contiguous spectrum asks for
// the mirrored order): read at every exec
inline bool one_rank_alternative(const dfft_plan *p) { return p->nranks == 1 && p->c2c && !p->opt.mirror && !p->spectral_mirror; }
// the launches of tunable pass k (fz fy fx ix iy iz) in the chain an exec would run now; nullptr where it runs none
std::vector<Launch> *pass_launches(dfft_plan *p, int k);
void graphs_clear(dfft_plan *p);     // drops the captured launch graphs (anything that changes the launches calls it)
