/*
 * dfft_c.h -- C ABI of libdfft_amd.so, the MI355X-native replacement for the hot path of
 * eggersn/DistributedFFT: "plan once, then execR2C / execC2R / (new) execC2C on device buffers".
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository).  The boundary is the abstract class
 *     template<typename T> class MPIcuFFT            include/mpicufft.hpp:55-105
 * and its concrete decompositions
 *     MPIcuFFT_Slab / _Slab_Opt1                      include/mpicufft_slab.hpp:99-125
 *     MPIcuFFT_Pencil / _Pencil_Opt1                  include/mpicufft_pencil.hpp:88-122
 * Differences by design: plain C, int return codes instead of printf+exit(EXIT_FAILURE)
 * (src/pencil/mpicufft_pencil_opt1.cpp:27-33), the communicator is an explicit dfft_comm
 * (RCCL over xGMI, in-process virtual ranks, or a caller-supplied all-to-all) instead of an
 * MPI_Comm, and complex-to-complex execution is added next to R2C/C2R.
 *
 * Memory layout contract (identical to the reference, README.md:247,
 * include/mpicufft_pencil.hpp:94-122): row-major [x][y][z], z contiguous.
 *   input  block of rank (i,j): [Nx/P1][Ny/P2][Nz]        (real for R2C, complex for C2C)
 *   output block of rank (i,j): [Nx][Ny/P1][Nzc/P2]       (complex; Nzc = Nz/2+1 or Nz)
 * Remainders of uneven divisions go to the lowest ranks.  rank = i*P2 + j.  Slab = P2 == 1.
 * Transforms are unnormalised, forward kernel exp(-2*pi*i*jk/N) (cuFFT convention).
 *
 * All functions return 0 on success; on failure a non-zero code and dfft_last_error() holds
 * a message (thread local).
 */
#ifndef DFFT_C_H
#define DFFT_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dfft_plan dfft_plan;
typedef struct dfft_comm dfft_comm;

/* which reference class the plan stands in for (all four share one engine: the "realigned"
 * opt1 data flow with pack/unpack fused into the FFT kernels; the value is kept for callers
 * that select by name and for the timer/CSV naming) */
enum dfft_kind {
    DFFT_SLAB = 0,         /* MPIcuFFT_Slab       include/mpicufft_slab.hpp          */
    DFFT_SLAB_OPT1 = 1,    /* MPIcuFFT_Slab_Opt1  include/mpicufft_slab_opt1.hpp     */
    DFFT_PENCIL = 2,       /* MPIcuFFT_Pencil     include/mpicufft_pencil.hpp        */
    DFFT_PENCIL_OPT1 = 3,  /* MPIcuFFT_Pencil_Opt1 include/mpicufft_pencil_opt1.hpp  */
    /* alternative slab sequence: 1-D z pass, one all-to-all, 2-D (y,x) pass.  Input split along x,
     * OUTPUT split along z: [Nx][Ny][Nzc/P] (include/mpicufft_slab_z_then_yx.hpp:41-44).  P2 must be 1. */
    DFFT_SLAB_Z_THEN_YX = 4,       /* MPIcuFFT_Slab_Z_Then_YX      include/mpicufft_slab_z_then_yx.hpp      */
    DFFT_SLAB_Z_THEN_YX_OPT1 = 5,  /* MPIcuFFT_Slab_Z_Then_YX_Opt1 include/mpicufft_slab_z_then_yx_opt1.hpp */
    /* forward only, like the reference: R2C along y, one all-to-all, 2-D (z,x) pass.  Output
     * [Nx][(Ny/2+1)/P][Nz] (include/mpicufft_slab_y_then_zx.hpp:40-43).  R2C plans: any Ny dfft_init accepts.  Unlike
     * the reference's single-rank branch (a z-Hermitian cufftPlan3d, mpicufft_slab_y_then_zx.cpp:111-121),
     * one rank produces the same y-Hermitian layout as several. */
    DFFT_SLAB_Y_THEN_ZX = 6        /* MPIcuFFT_Slab_Y_Then_ZX      include/mpicufft_slab_y_then_zx.hpp      */
};
enum dfft_precision { DFFT_F32 = 0, DFFT_F64 = 1 };   /* template parameter T = float|double */
enum dfft_direction { DFFT_FORWARD = -1, DFFT_INVERSE = 1 };
/* third "direction" of the debug interface (dfft_debug_get_chain, dfft_debug_trace_chain): the chain of dfft_exec_spectral_op */
#define DFFT_SPECTRAL_OP 2
#define DFFT_SPECTRAL_OPS 3          /* debug "direction": the multi-output chain for the option's value */
#define DFFT_SPECTRAL_MAX_OUTPUTS 8
#define DFFT_SPECTRAL_SUM 4          /* debug "direction": the multi-input chain (dfft_exec_spectral_sum) for the option's value */
#define DFFT_SPECTRAL_MAX_INPUTS 8

/* struct Configurations, include/params.hpp:83-93.  comm/send method enums are accepted and
 * recorded; the device exchange always runs as one grouped all-to-all per exchange. */
typedef struct dfft_config {
    int cuda_aware;        /* kept for source compatibility; device buffers are always used */
    int warmup_rounds;
    int comm_method;       /* 0 Peer2Peer, 1 All2All   (params.hpp:83) */
    int send_method;       /* 0 Sync, 1 Streams, 2 MPI_Type (params.hpp:84) */
    int comm_method2;
    int send_method2;
} dfft_config;

/* ---------------------------------------------------------------- communicators ---------- */
/* replaces MPI_Comm + MPI_Comm_split (src/mpicufft.cpp:42-51, mpicufft_pencil_opt1.cpp:103-104) */

/* all-to-all-v callback: byte counts/displacements, `group` = global ranks of the members,
 * `me` = caller's index in group.  Buffers are device pointers; `stream` is the hipStream_t
 * the plan enqueues on.  Must return 0 on success. */
typedef int (*dfft_alltoallv_fn)(void *user, const void *sendbuf, const size_t *sendcounts,
                                 const size_t *sdispls, void *recvbuf, const size_t *recvcounts,
                                 const size_t *rdispls, const int *group, int ngroup, int me,
                                 void *stream);

/* Optional second callback of a callback communicator: a schedule of point-to-point pieces over the WHOLE communicator as one
 * grouped operation (the two hops of the relay, see "relay" below: several pieces per peer, not back to back).  Piece i of the send
 * list goes to global rank speer[i], piece j of the receive list comes from rpeer[j]; pointers are absolute; the pieces between two
 * ranks appear in the same order at both ends (match them in that order: grouped ncclSend / ncclRecv, torch.distributed
 * batch_isend_irecv, MPI_Isend / MPI_Irecv with the position as the tag).  Must return 0 on success.  Without it the library runs a
 * schedule as group_size - 1 all-to-all-v callbacks. */
typedef int (*dfft_sendrecv_list_fn)(void *user, int nsend, const int *speer, void *const *sptr, const size_t *sbytes, int nrecv,
                                     const int *rpeer, void *const *rptr, const size_t *rbytes, void *stream);

/* nranks virtual ranks inside this process sharing the current device; each rank's exec must be
 * called from its own host thread (they meet in a barrier like MPI ranks would). */
int dfft_comm_create_local(int nranks, dfft_comm **world);
/* one process per GPU over RCCL/xGMI; id = 128-byte ncclUniqueId made on rank 0 by
 * dfft_rccl_unique_id and broadcast by the caller (MPI_Bcast, torch.distributed, ...) */
int dfft_rccl_unique_id(void *id128);
int dfft_comm_create_rccl(const void *id128, int nranks, int rank, dfft_comm **comm);
/* caller-supplied exchange (e.g. torch.distributed.all_to_all_single, MPI_Alltoallv) */
int dfft_comm_create_callback(int nranks, int rank, dfft_alltoallv_fn fn, void *user, dfft_comm **comm);
int dfft_comm_set_list_callback(dfft_comm *comm, dfft_sendrecv_list_fn fn, void *user);
/* nranks = the size the communicator was created with; transport_nranks = what the transport itself reports
 * (ncclCommCount for the RCCL transport, 0 for the others), so that a caller can verify that RCCL really
 * spans the ranks it claims */
int dfft_comm_info(const dfft_comm *comm, int *nranks, int *transport_nranks);
/* What went through a communicator since it was made: "alltoallv" (all-to-all-v operations of the transport: the direct exchanges, the
 * relay's table gathers, the layers of a schedule on a transport without a native form), "list" (native point-to-point schedules:
 * one per hop of a relayed exchange), "relayed" (relayed exchanges), "relay_meta" (table gathers: one per exchange table).  A relayed
 * exchange of one pipeline chunk is 2 "list" operations on the RCCL, the local-world and the torch transport. */
int dfft_comm_get_counter(const dfft_comm *comm, const char *name, long *value);
/* transport knobs.  "dup_channel" = 1 (RCCL transport only; COLLECTIVE -- every rank of the communicator calls it at
 * the same point): duplicate the communicator (ncclCommSplit) for the second exchange of pencil plans, so that the row-
 * and the column-group exchange -- which use disjoint xGMI links -- may be on the wire at the same time; without it one
 * ncclComm serialises them.  "dup_channel" = 3: two more duplicates for the relay's first hop of either exchange, which then
 * overlaps the second hop of the previous pipeline chunk ("relay_overlap").  Replaces nothing in the reference (its two MPI sub-communicators are independent by
 * construction, src/pencil/mpicufft_pencil_opt1.cpp:103-104).
 * "self_send" = 1 (RCCL transport, testing): a rank's own block goes through ncclSend / ncclRecv to itself instead of a device
 * copy, so that a single-GPU box can hand caller buffers (virtual-memory ranges from dfft_malloc included) to RCCL.
 * "relay" = 0..3 (every transport; a flag, not collective by itself, but every rank must set the same value before the next
 * exec): two-hop relay of the group exchanges.  bit 0 = exchange 2 (column groups), bit 1 = exchange 1 (row groups).  xGMI is
 * point to point, so the column groups of a 2 x 4 pencil grid move half of the volume over ONE of a GPU's seven links; with the
 * relay a message is cut into nranks parts, two travel directly and each of the others through one of the ranks outside the
 * pair.  All partners of an exchange travel together: TWO grouped transport operations per exchange and pipeline chunk (hop 1: every
 * link carries one part of each of the rank's messages; hop 2: the second direct parts and everything staged goes on to its
 * destination), all links equally loaded in both (1 GiB over one link: 7.0 -> 1.75 ms at 153 GB/s per link).  The bytes
 * land exactly where the direct exchange puts them.  "relay_overlap" = 1 (default) / 0: hop 1 of a pipeline chunk runs on a side
 * stream (on the RCCL transport: on its own communicator if "dup_channel" = 3 made one) under hop 2 of the chunk before it.  The reference's answer to its slow exchanges was per-peer overlap
 * (src/pencil/mpicufft_pencil_opt1.cpp:1116-1275); this is the xGMI analogue.  Default off.
 * Returns 0, or nonzero for an unknown key / a failure. */
int dfft_comm_set_option(dfft_comm *comm, const char *key, long value);
/* The transport's all-to-all-v on its own -- what a plan calls for its exchanges (counts / displacements in bytes, `group` =
 * ranks of the communicator taking part, `me` = the caller's index in it; hip_stream may be NULL).  Stream-ordered: returns
 * when the exchange is enqueued.  For callers that move their own blocks with the library's transports, and for tests of a
 * transport by itself (the reference's counterpart is a bare MPI_Alltoallv, src/pencil/mpicufft_pencil_opt1.cpp:784-785). */
int dfft_comm_alltoallv(dfft_comm *comm, int myrank, const void *send, const size_t *scounts, const size_t *sdispls, void *recv,
                        const size_t *rcounts, const size_t *rdispls, const int *group, int ngroup, int me, void *hip_stream);
/* The transport's point-to-point schedule on its own -- what the relay calls for each of its two hops: piece i of the send list goes
 * to rank speer[i], piece j of the receive list comes from rpeer[j]; `slayer` / `rlayer` number the pieces between one ordered pair of
 * ranks (both ends give a piece the same layer, at most one piece per peer, direction and layer; nlayers the same on all ranks).  One
 * grouped operation on the RCCL, local-world and list-callback transports, nlayers all-to-all-v calls elsewhere.  COLLECTIVE over the
 * communicator.  Stream-ordered.  Option "test_channel" = 0..3 picks the channel (communicator) the two bare calls use. */
int dfft_comm_sendrecv_list(dfft_comm *comm, int myrank, int nsend, const int *speer, const int *slayer, void *const *sptr, const size_t *sbytes,
                            int nrecv, const int *rpeer, const int *rlayer, void *const *rptr, const size_t *rbytes, int nlayers, void *hip_stream);
/* destroy the plans that use a communicator before the communicator itself */
int dfft_comm_destroy(dfft_comm *comm);

/* ---------------------------------------------------------------- plan -------------------- */
/* MPIcuFFT<T>::MPIcuFFT(Configurations, MPI_Comm, int max_world_size)   src/mpicufft.cpp:42-66.
 * comm may be NULL for a single rank.  `rank` selects the virtual rank of a local world and is
 * ignored (taken from the comm) otherwise.  max_world_size < 0 = all ranks. */
int dfft_plan_create(dfft_plan **plan, int kind, int precision, const dfft_config *config,
                     dfft_comm *comm, int rank, int max_world_size);
/* ~MPIcuFFT  src/mpicufft.cpp:68-73 (frees the work area if the library allocated it) */
int dfft_plan_destroy(dfft_plan *plan);

/* initFFT(GlobalSize*, Partition*, bool allocate)   include/mpicufft.hpp:60,
 * src/pencil/mpicufft_pencil_opt1.cpp:46-326, src/slab/default/mpicufft_slab.cpp:97-281.
 * P1*P2 must equal the number of ranks.  Axis lengths: powers of two up to 8192 (4096 on the real axis of an R2C
 * plan) and the lengths 2^a 3^b 5^c 7^d <= 2048 listed in csrc/kernels_mixed.inc (native chain), any other length
 * up to 4096 (Bluestein), and beyond that every length N1*N2 <= 2^24 whose factors are each such a length (two-level
 * lines: two launches per pass and a scratch region in the work area, dfft_axis_plan_info shows the split); a length
 * that does not split that way (a prime above 4096, twice such a prime ...) runs Bluestein's algorithm over a two-level padded
 * length (four launches), so every length from 2 to 2^23 has a plan; beyond 2^24 points per line: ERR_UNSUPPORTED.  c2c = 0: R2C/C2R plan (Nz_out = Nz/2+1,
 * include/params.hpp:30); c2c = 1: complex plan (Nz_out = Nz).  Option "spectral_op" narrows the x length: 1 = a power of two up to 2048,
 * 2 = that or a mixed-radix length with a fused kernel (dfft_spectral_op_supported); ERR_UNSUPPORTED otherwise. */
int dfft_init(dfft_plan *plan, size_t Nx, size_t Ny, size_t Nz, int P1, int P2, int c2c, int allocate);
/* setWorkArea(void *device, void *host)   mpicufft_pencil_opt1.cpp:329-387.  NULL device =
 * library allocates dfft_work_size_device() bytes. */
int dfft_set_work_area(dfft_plan *plan, void *device, void *host);
/* Pipeline depth of the exchanges: every pass that feeds an all-to-all is cut into `chunks`
 * pieces so that chunk c travels (communication stream) while chunk c+1 is transformed (compute
 * stream).  The reference's counterpart is the Peer2Peer overlap of
 * src/pencil/mpicufft_pencil_opt1.cpp:601-754.  Takes effect at the next dfft_init; 0 = default (4 when the
 * plan has an exchange, else 1), 1 = no pipelining = the reference's exact message sizes. */
int dfft_set_pipeline_chunks(dfft_plan *plan, int chunks);
int dfft_get_pipeline_chunks(const dfft_plan *plan);
/* Tuning knobs, by name (takes effect at the next dfft_init unless noted).  The reference's counterpart is the
 * Configurations struct (include/params.hpp:85-93); these are the knobs this engine has instead:
 *   "pipeline_chunks"  as dfft_set_pipeline_chunks                      (env default DFFT_CHUNKS)
 *   "mirror_inverse"   1: a single-rank complex inverse runs the multi-rank pass order x, y, z instead of the
 *                      forward order with conjugation (next exec; benchmarking the N > 1 compute path on one GPU;
 *                      env default DFFT_MIRROR)
 *   "point_tables"     per-point address tables: 0 never, 1 segmented sides (default), 2 always (DFFT_TABLES)
 *   "shift"            row-aligned tile windows for odd-pitch output rows: -1 auto, 0 off, 2 always (DFFT_SHIFT)
 *   "single_order"     one rank, complex plan: 1 = pass order z, x, y through a padded private layout, 0 = z, y, x, -1 (default)
 *                      = where it measured faster (env default DFFT_SINGLE_ORDER); "single_layout" (0 | 1) and "single_pad"
 *                      (bytes) shape that layout
 *   "spectral_layout"  0 (default): the spectrum has the reference's layout [Nx][yo][zs] (include/mpicufft_pencil.hpp:94-122).  1: it is kept
 *                      x-contiguous, [yo][zs][Nx] -- entry (kx, ky, kz') at kx + Nx * (kz' + zs * ky), dfft_get_out_strides -- so
 *                      that the forward x pass stores natural lines and the inverse x pass loads them: neither touches the
 *                      point-major layout, whose strided read (16-byte points Nx rows apart) is the slowest pass of every multi-rank
 *                      plan.  For callers that go forward -> pointwise work on the spectrum -> inverse (the reference's testcase 4,
 *                      tests/src/pencil/random_dist_3D.cu:748-793, does exactly that) and can index through the strides.
 *                      getOutSize / getOutStart / the exchange tables are unchanged.  Pencil and default slab plans, any rank count.
 *   "spectral_op"      0 (default) | 1 | 2, before dfft_init: the plan also builds what dfft_exec_spectral_op runs -- forward transform,
 *                      pointwise multiplier, inverse transform as ONE chain whose forward and inverse x passes are a single launch
 *                      (the spectrum never reaches memory).  It costs one more domain-sized slice of the work area
 *                      (dfft_work_size_device reports it) and nothing else: with 0 no size, launch or chain of the plan differs.  Pencil
 *                      and default slab plans, any rank count, both "spectral_layout" settings, C2C and R2C; the x length must be a power
 *                      of two up to 2048 (dfft_init: ERR_UNSUPPORTED otherwise, and for the Z_Then_YX / Y_Then_ZX sequences).
 *                      2: everything 1 is, and the x length may also be one of the mixed-radix lengths 2^a 3^b 5^c 7^d <= 2000 that have a
 *                      fused kernel in libdfft_amd_any.so (384, 768, 1000, 1536, ...: dfft_spectral_op_supported; DESIGN.md lists the few
 *                      native lengths left out), running the native chain -- ERR_UNSUPPORTED for an x length on the Bluestein or
 *                      two-level kernel ("native_mixed" = 0, "two_level" = 1, any other length).  A power-of-two x length gives the same
 *                      plan under 1 and 2.  Any other value: ERR_ARG.
 *   "spectral_outputs" 1 (default) .. 8 (DFFT_SPECTRAL_MAX_OUTPUTS), before dfft_init; from 2 on it needs "spectral_op" = 1 or 2.  K >= 2: the
 *                      plan also builds the chain of dfft_exec_spectral_ops -- one forward half (z, y, both exchanges), then per output
 *                      the fused x launch with that output's operator and the inverse y and z passes with their exchanges -- out of the
 *                      launches it already has.  It costs at most one more domain-sized slice of the work area, the same for every K
 *                      (dfft_work_size_device reports it; none on a P1 x P2 pencil with both factors above 1), because that chain never
 *                      overwrites the slice the fused launch reads.  With 1 no size, launch or chain of the plan differs.  Any other
 *                      value, or K >= 2 without "spectral_op": ERR_ARG at dfft_init.
 *   "spectral_inputs"  1 (default) .. 8 (DFFT_SPECTRAL_MAX_INPUTS), before dfft_init; from 2 on it needs "spectral_op" = 1 or 2.  K >= 2: the
 *                      plan also builds the chain of dfft_exec_spectral_sum -- per input the z and y passes with their exchanges and
 *                      the fused x launch with that input's operator, which from the second input on ADDS its result to the first's,
 *                      then ONE inverse half -- out of the launches it already has.  It costs one more domain-sized slice of the work
 *                      area on every grid, the accumulator, the same for every K (dfft_work_size_device reports it); a plan that also
 *                      sets "spectral_outputs" >= 2 pays for one extra slice in total, the two chains share it.  With 1 no size, launch
 *                      or chain of the plan differs.  Any other value, or K >= 2 without "spectral_op": ERR_ARG at dfft_init.
 *   "graph"            1: a single-rank plan replays the kernel launches of an exec as one hipGraph from the second call
 *                      with the same (operation, in, out) on; 0 (default): plain launches -- measured 6-8 us faster per
 *                      exec on ROCm 7.2 (profiles/r2_graph_latency.txt)
 *                      Such a plan runs on its own stream alone (no second compute stream): only that stream is captured.
 *   "compute_streams"  2: the pipeline chunks of a pass alternate over two compute streams (chunk c on stream c mod 2), so that the
 *                      drain of one chunk overlaps the ramp of the next; 1: one stream; -1 (default): two from three chunks per pass
 *                      on.  Read at every exec: it takes effect at the NEXT EXEC, also when it is set after dfft_init and after
 *                      dfft_set_work_area (the second stream is created by the first exec that needs it).  Never two streams while
 *                      two-level or long-Bluestein passes share the plan's level scratch, under "graph", or at a pipeline depth of 1;
 *                      dfft_debug_trace_chain shows what the next exec does.
 *   "trace"            debug, 0 (default) | 1: every exec keeps the list of the launches, exchanges, event records and stream waits
 *                      it issued, readable through dfft_debug_trace_chain(plan, direction, 0, ...) (next exec)
 *   "native_mixed"     1 (default): lengths that are not powers of two but have a mixed-radix configuration run the
 *                      native chain; 0: they run the Bluestein kernel like every other length (A/B runs, tests)
 *   "debug_skip"       measurement only, a bit set: bit 0 (value 1) = every pass skips its transform and becomes a copy with
 *                      the same access pattern (results are wrong); used to measure the pattern's own roofline.  Bit 1
 *                      (value 2) = the closed-form address sides compute per-point 64-bit vector addresses instead of a scalar
 *                      base + 32-bit lane offset (same results bit for bit; A/B of the address forms)
 *   "variant_<pass>", "order_<pass>", "real_variant"   kernel configuration / workgroup order per pass
 *                      (<pass> = fz fy fx ix iy iz; -1 = the plan's choice), for A/B measurements
 * Returns nonzero for an unknown key.  dfft_get_option returns -1 for an unknown key. */
int dfft_set_option(dfft_plan *plan, const char *key, long value);
long dfft_get_option(dfft_plan *plan, const char *key);
/* HIP stream all kernels/exchanges are enqueued on (default: a non-blocking stream owned by the
 * plan).  exec orders itself only against this stream: work that produces `in` or initialises
 * `out` on another stream must be complete (or that stream handed over here) before exec. */
int dfft_set_stream(dfft_plan *plan, void *hip_stream);

/* execR2C(void *out, const void *in)   include/mpicufft.hpp:63; mpicufft_pencil_opt1.cpp:1422-1519.
 * in: device, real [xs][ys][Nz], not modified.  out: device, >= dfft_domain_size() bytes;
 * holds [Nx][yo][zs] complex on return.  Blocking (returns after the stream is drained), like
 * the reference's trailing cudaDeviceSynchronize.
 * Footprint of every exec entry point (tests/test_gpu_footprint.py holds each of them to it on guarded buffers): an exec reads and
 * writes inside `in`, `out` and the dfft_work_size_device() bytes of the work area and nowhere else, and its result does not depend
 * on what `out` or the work area held before.  Alignment: every device pointer (in, out, the work area, multiplier arrays and
 * tables) must be aligned to 16 bytes, the size of an fp64 complex point.  Beyond that alignment is a matter of speed only: tile
 * windows and their cache-line shifts are computed relative to the buffer's base, and they fill whole 128-byte lines when the base
 * is 128-byte aligned, as every hipMalloc result and the 256-byte-aligned slices of the library's own work area are.  (The tests run
 * buffers at 2 MiB alignment and, for the ragged and odd-pitch cases, again 256 bytes off it.) */
int dfft_exec_r2c(dfft_plan *plan, void *out, const void *in);
/* execC2R(void *out, const void *in)   include/mpicufft_pencil.hpp:106-111; :1522-1600.
 * `in` is DESTROYED (used as scratch, as in the reference :1534,1544,1563): it must hold dfft_domain_size() bytes, like the `out`
 * of the forward transform that filled it.  out: the input block [xs][ys][Nz], real; exactly its size is written, no more is needed. */
int dfft_exec_c2r(dfft_plan *plan, void *out, void *in);
/* new: complex-to-complex, same layouts with Nz_out = Nz.  Forward: in [xs][ys][Nz] -> out
 * [Nx][yo][zs].  Inverse: in [Nx][yo][zs] (destroyed) -> out [xs][ys][Nz].
 * Forward: `in` is not modified (the pointer is not const because the inverse shares the entry point); out >= dfft_domain_size()
 * bytes.  Inverse: `in` must hold dfft_domain_size() bytes (scratch); out: the input block's size, xs * ys * Nz complex, is enough. */
int dfft_exec_c2c(dfft_plan *plan, void *out, void *in, int direction);
/* partial transforms: execR2C(out, in, d) / execC2R(out, in, d) of MPIcuFFT_Pencil
 * (include/mpicufft_pencil.hpp:101-111, src/pencil/mpicufft_pencil.cpp:1644-1839).  Works for
 * R2C and C2C plans alike (the plan decides).  d = 3: the full transform.  d = 1: z axis only,
 * stage layout [xs][ys][Nzc] (natural, z contiguous).  d = 2: z then y, stage layout
 * [xs][Ny][zs].  The inverse direction takes those layouts as input and returns [xs][ys][Nz].
 * Forward (every d): `in` is not modified; the stage layouts are never larger than dfft_domain_size() bytes, which is what `out`
 * must hold.  Inverse, d = 1, 2: `in` holds the stage layout and may be used as scratch like that of the full inverse; out: the
 * input block's size (xs * ys * Nz real resp. complex entries) is enough. */
int dfft_exec_dim(dfft_plan *plan, void *out, void *in, int direction, int d);
/* non-blocking variants: enqueue only (caller synchronises the stream) */
int dfft_enqueue_c2c(dfft_plan *plan, void *out, void *in, int direction);

/* new: out = IFFT(m * FFT(in)), unnormalised (times Nx*Ny*Nz; fold 1/(Nx*Ny*Nz) into `scale`), in one call -- the loop of the reference's
 * testcase 4 (tests/src/pencil/random_dist_3D.cu:685-811: forward, multiply by -|k|^2, inverse).  `in` and `out` are both blocks of the
 * INPUT layout [xs][ys][Nz] (real for an R2C plan); `in` is only read, out == in is refused (ERR_ARG).  The last forward pass and the first
 * inverse pass both work on complete x lines of one rank, so they run as one kernel with the multiplier between them: 11 (array) or 10
 * (real and complex tables) trips of a domain-sized buffer through memory instead of the 15 of exec_r2c + a pointwise kernel + exec_c2r.
 * The multiplier m(kx, ky, kz) over the rank's spectrum block (dfft_get_out_size / dfft_get_out_start):
 *   kind 0  scale * mult[...]: a complex device array of the plan's precision in the layout of the spectrum block, i.e. indexed through
 *           dfft_get_out_strides ([Nx][yo][zs], or [yo][zs][Nx] with "spectral_layout" = 1)
 *   kind 1  scale * (ax[kx] + ay[ky] + az[kz]): three real device tables of the plan's precision with Nx, yo, zs entries, local to the
 *           block (entry 0 of ay is global ky = out_start[1])
 *   kind 2  scale / (ax[kx] + ay[ky] + az[kz]), and 0 where the sum is 0 (a Poisson solve next to kind 1's Laplacian)
 *   kind 3  scale * P, P = cx[kx] * cy[ky] * cz[kz]: three COMPLEX device tables of the plan's precision with Nx, yo, zs entries, local to
 *           the block exactly as ax, ay, az are (entry 0 of cy is global ky = out_start[1]).  A NULL table is a factor of 1; at least one of
 *           the three must be non-NULL (ERR_ARG).  A derivative i*kx, a Gaussian filter, a translation exp(i k.d): every separable multiplier
 *           at the traffic of the table forms (10 trips) and Nx + yo + zs entries of memory
 *   kind 4  scale * P * (ax[kx] + ay[ky] + az[kz])                   (all of ax, ay, az, like kinds 1 and 2)
 *   kind 5  scale * P / (ax[kx] + ay[ky] + az[kz]), and 0 where the sum is 0 (one component of the gradient of a Poisson solution:
 *           cx = i*kx, the sums -|k|^2)
 * cx, cy, cz were appended to the struct: kinds 0 .. 2 never read them, so a caller compiled against the six-field struct stays correct.
 * The plan must have been initialised with option "spectral_op" = 1 or 2 (ERR_STATE otherwise; 2 admits mixed-radix x lengths).  Blocking, like dfft_exec_r2c; collective on a
 * multi-rank plan.  No phase timing and no hipGraph replay for this chain. */
typedef struct dfft_spectral_op {
    int32_t kind;           /* 0 array, 1 sum of tables, 2 reciprocal of the sum of tables, 3 product of factor tables, 4 product * sum,
                             * 5 product / sum */
    double scale;
    const void *mult;       /* kind 0 */
    const void *ax, *ay, *az;   /* kind 1, 2, 4, 5 */
    const void *cx, *cy, *cz;   /* kind 3, 4, 5 (read for no other kind) */
} dfft_spectral_op;
int dfft_exec_spectral_op(dfft_plan *plan, void *out, const void *in, const dfft_spectral_op *op);
/* new: several operators on one input, outs[j] = IFFT(ops[j] * FFT(in)) for j < nout -- the components of a gradient, a field and its
 * Laplacian -- with ONE forward half: the z and y passes and both forward exchanges run once, the fused x launch and the inverse half
 * once per output.  4 + 6 nout trips of a domain-sized buffer through memory and 2 + 2 nout exchanges instead of the 10 nout and 4 nout
 * of nout calls of dfft_exec_spectral_op (table forms), and every outs[j] is bit for bit what that call gives.  The plan needs
 * option "spectral_outputs" >= nout (ERR_STATE while the option is 1: "set spectral_outputs before dfft_init"); nout = 1 is valid on such a
 * plan.  Every outs[j] is a block of the input layout like `out` above; `in` is only read.  Footprint: `in`, the outs[j] and the
 * dfft_work_size_device() bytes of the work area.  ERR_ARG: nout < 1 or above the option's value, a null pointer, two equal outputs, an
 * output equal to `in`, an ops[j] that dfft_exec_spectral_op would refuse (the message names j; the same checks, the 32-bit lane-offset
 * bound of kind 0 included: ERR_UNSUPPORTED).  Blocking; collective on a multi-rank plan, every rank with the same nout. */
int dfft_exec_spectral_ops(dfft_plan *plan, int nout, void *const *outs, const void *in, const dfft_spectral_op *ops);
/* new: several inputs summed into one output, out = sum_j IFFT(ops[j] * FFT(ins[j])) for j < nin, unnormalised like
 * dfft_exec_spectral_op -- the divergence of a vector field (3 -> 1), a component of a curl (2 -> 1), the pressure right-hand side of a
 * Navier-Stokes step -- with ONE inverse half: the inverse transform is linear, so the sum is taken in spectral space.  Per input the z
 * and y passes, both forward exchanges and the fused x launch run; the fused launch of input 0 stores its result t_0 to a work slice, that
 * of every later input adds to it IN THE ORDER j = 0, 1, ...: ((t_0 + t_1) + t_2) ..., one rounding per addition; then exchange 2
 * backwards and the inverse y and z passes run once.  7 nin + 3 trips of a domain-sized buffer through memory and 2 nin + 2 exchanges
 * instead of the 10 nin and 4 nin of nin calls of dfft_exec_spectral_op plus the caller's pointwise sum and nin - 1 temporaries
 * (DESIGN.md).  With nin = 1 the result is bit for bit that of dfft_exec_spectral_op.  The operators are the table forms, kinds 1 .. 5;
 * kind 0 (an array) is refused with ERR_UNSUPPORTED: it would take nin domain-sized multiplier arrays and has no accumulating kernel.
 * The plan needs option "spectral_inputs" >= nin (ERR_STATE while the option is 1: "set spectral_inputs before dfft_init"); nin = 1 is
 * valid on such a plan.  Every ins[j] and `out` is a block of the input layout; the inputs are only read, and two equal inputs (with
 * different operators) are allowed.  Footprint: the ins[j], `out` and the dfft_work_size_device() bytes of the work area.  ERR_ARG:
 * nin < 1 or above the option's value, a null pointer, `out` equal to an input, an ops[j] that dfft_exec_spectral_op would refuse (the
 * message names ops[j]).  A refused call writes nothing.  Blocking; collective on a multi-rank plan, every rank with the same nin.  No
 * phase timing and no hipGraph replay for this chain. */
int dfft_exec_spectral_sum(dfft_plan *plan, void *out, int nin, const void *const *ins, const dfft_spectral_op *ops);
/* 1 if dfft_init with default options accepts an x length of Nx points under option "spectral_op" = option_value (1 or 2), else 0
 * (also for another option_value or precision).  Host only: no device is touched; loads libdfft_amd_any.so when Nx is not a power of two. */
int dfft_spectral_op_supported(int precision, size_t Nx, int option_value);

/* getInSize/getInStart/getOutSize/getOutStart   include/mpicufft_pencil.hpp:112-122
 * (getOutStart returns start_z of the z split -- the reference indexes start_x there, a bug) */
int dfft_get_in_size(const dfft_plan *plan, size_t size[3]);
int dfft_get_in_start(const dfft_plan *plan, size_t start[3]);
int dfft_get_out_size(const dfft_plan *plan, size_t size[3]);
int dfft_get_out_start(const dfft_plan *plan, size_t start[3]);
/* getPartitionDimensions(input_dim, transposed_dim, output_dim)   include/mpicufft_pencil.hpp:112-116, tables of
 * struct Partition_Dimensions (include/params.hpp:58-81) as built in src/pencil/mpicufft_pencil_opt1.cpp:70-93.
 * which = 0 input_dim, 1 transposed_dim, 2 output_dim; axis = 0 x, 1 y, 2 z.  Writes the per-rank extents and
 * offsets of that axis at that stage (one entry = the full extent when the axis is not split there); *count
 * receives the number of entries, at most `capacity` are written (sizes/starts may be NULL to query). */
/* element strides of the spectrum block in `out` along (kx, ky_local, kz_local): entry (kx, ky, kz) of the block dfft_get_out_size
 * describes lives at kx * s[0] + ky * s[1] + kz * s[2].  {yo * zs, zs, 1} for the reference layout, {1, zs * Nx, Nx} with option
 * "spectral_layout" = 1. */
int dfft_get_out_strides(const dfft_plan *plan, size_t s[3]);
int dfft_get_partition_dimensions(const dfft_plan *plan, int which, int axis, size_t *sizes, size_t *starts,
                                  size_t capacity, size_t *count);
/* getDomainSize / getWorkSizeDevice / getWorkSizeHost / getRank / getWorldSize
 * include/mpicufft.hpp:65-78 */
size_t dfft_domain_size(const dfft_plan *plan);        /* bytes `out` must hold */
size_t dfft_work_size_device(const dfft_plan *plan);
size_t dfft_work_size_host(const dfft_plan *plan);
void *dfft_work_area_device(const dfft_plan *plan);
int dfft_rank(const dfft_plan *plan);
int dfft_world_size(const dfft_plan *plan);

/* exchange tables in BYTES exactly as the reference builds them for MPI_Alltoallv
 * (mpicufft_pencil_opt1.cpp:269-273 which=1, :315-319 which=2).  Arrays hold P2 resp. P1 entries. */
int dfft_get_exchange_tables(const dfft_plan *plan, int which, size_t *sendcounts, size_t *sdispls,
                             size_t *recvcounts, size_t *rdispls);
/* run only exchange `which` (1 = row group, 2 = column group) of the plan on caller buffers,
 * forward (send tables) or inverse (tables swapped) direction, blocking.  This is the
 * MPI_Alltoallv step of the reference in isolation (:784-785 / :829-830, :1297-1298 / :1341-1342);
 * used by the transport tests. */
int dfft_exchange(dfft_plan *plan, int which, int direction, const void *sendbuf, void *recvbuf);
/* the tables the pipelined exchanges actually use: chunk `chunk` (0 .. dfft_get_pipeline_chunks-1) of
 * exchange `which`, for the forward or the inverse transform, in send/recv order of that direction
 * (bytes; displacements are absolute offsets in the send resp. receive buffer).  Over all chunks
 * the counts add up to dfft_get_exchange_tables(). */
int dfft_get_pipeline_tables(const dfft_plan *plan, int direction, int which, int chunk, size_t *sendcounts,
                             size_t *sdispls, size_t *recvcounts, size_t *rdispls);
/* lines interleaved per tile in the intermediate layouts */
int dfft_tile_lines(const dfft_plan *plan);

/* per-phase device time of the last exec in milliseconds (Timer sections of the reference,
 * include/mpicufft_pencil.hpp:263-287): up to 8 entries, names via dfft_phase_name */
int dfft_get_phase_times(dfft_plan *plan, float *ms, int max_entries);
const char *dfft_phase_name(int phase, int direction);
int dfft_enable_phase_timing(dfft_plan *plan, int enable);

/* standalone launch of one batched 1-D axis pass on natural lines (in [batch][N] -> out
 * [batch][N]); used by the kernel-level parity tests and the micro-benchmarks */
int dfft_fft1d_batched(int precision, size_t N, size_t batch, void *out, const void *in,
                       int direction, void *hip_stream);

/* same with an explicit kernel configuration (0 = default; unknown values fall back to 0; -1 = the Bluestein kernel
 * even where the length has a native configuration) and the measurement-only debug flags of "debug_skip" */
int dfft_fft1d_batched_ex(int precision, size_t N, size_t batch, void *out, const void *in, int direction,
                          void *hip_stream, int variant, int debug);

/* ---- introspection of the pass descriptors (host only; used by the CPU layout tests) -------- *
 * One axis pass of the plan: which lines it transforms and the address forms of its load and store
 * side (enum values as in distributedfft_amd/csrc/fft_pass.hip.h).  Offsets
 * are in ELEMENTS of the side's type except in_off / out_off (bytes added to the stage buffer). */
typedef struct dfft_pass_desc {
    uint32_t na, LB, nb, LA, T2shift;
    int32_t load_kind;      /* 0 natural lines, 1 tiled (segments), 2 point-major (KS_in, AS_in) */
    int32_t store_kind;     /* 0 lines (row strides if KS_out != 0), 1 point-major, 2 tiled-same, 3 tiled-transpose */
    int32_t swap, shift;
    uint64_t KS_in, KS_out, AS_in, AS_out;      /* load_kind 0 with KS_in != 0: rows a*AS_in + line*KS_in (strided natural lines) */
    uint64_t IA, IB;        /* tiled load, one segment: explicit strides of a and of a tile along b (0 = packed) */
    uint64_t SK, SB;        /* tiled-same store: explicit strides of a point k and of a tile along b (0 = packed) */
    int32_t a_fastest, xcd_swizzle;
    uint64_t in_off, out_off;
    int32_t lnseg, snseg;
    uint32_t lstart[32], llen[32];
    uint64_t lbase[32];
    uint32_t sstart[32], slen[32];
    uint64_t sbase[32];
} dfft_pass_desc;
/* What every pass of the plan runs with right now -- the rules of dfft_init, or what dfft_tune_variants / dfft_tune_placement kept:
 * passes in the order fz fy fx ix iy iz; variant = kernel configuration number (the role numbers of csrc/cfg_f64.hip.h / cfg_f32.hip.h),
 * order = a_fastest + 2 * xcd_swizzle of the workgroup -> tile mapping, addr64 = 1 where the pass keeps per-point 64-bit vector
 * addresses.  Any of the arrays may be NULL.  (A caller can pin the same choices on another plan with the "variant_<pass>" /
 * "order_<pass>" options.) */
int dfft_get_pass_choices(const dfft_plan *plan, int variant[6], int order[6], int addr64[6]);
/* name: "fz" "fy" "ix" "iy" "iz" "py2" "qy2" "xx" "zy" "ziy" (index = chunk, or chunk*P + peer for zy/ziy; "xx": option "spectral_op")
 * and "fx" "zix" "yz" "pz1" "qz1" "sz" "sx" "sy" (index 0; the last three: single-rank complex plans, order z, x, y).  Returns nonzero if the plan has no such launch. */
int dfft_debug_get_pass(const dfft_plan *plan, const char *name, int index, dfft_pass_desc *desc);
/* One step of the chain an exec would run now (dfft_debug_get_chain): the launches of a group, chunk by chunk, each chunk followed by
 * the exchange, if any.  Chunk c runs the group's launches c*per_chunk .. (c+1)*per_chunk - 1. */
typedef struct dfft_chain_step {
    char group[8];          /* launch group, as dfft_debug_get_pass names it */
    int32_t axis;           /* 0 z, 1 y, 2 x */
    int32_t launches, per_chunk;
    int32_t src, dst;       /* -2 the exec's input (input 0 of dfft_exec_spectral_sum; -(9 + j): its input j >= 1), -1 its output (output 0
                             * of dfft_exec_spectral_ops; -(2 + j): its output j >= 1), k >= 0 slice k of the work area (dfft_domain_size
                             * bytes each) */
    int32_t conj;           /* 1: launched with conjugation whatever the descriptor's swap says */
    int32_t form;           /* 0 / 1 / 2 complex lines (forward / inverse / fixed kernel configuration), 3 real z lines in (R2C),
                             * 4 real z lines out (C2R), 5 real strided lines in (R2C), 6 as 2 with the result ADDED to what dst holds
                             * (the "xx" steps of inputs j >= 1 of dfft_exec_spectral_sum: the launch reads and writes dst) */
    int32_t exchange;       /* 0, or 1 / 2: that exchange after every chunk, dst -> the next step's src, with the tables
                             * dfft_get_pipeline_tables reports for the exec's direction */
    int32_t split;          /* the same for every step of a chain: 1 if its chunks may alternate over two compute streams (option
                             * "compute_streams") */
    int32_t tables;         /* DFFT_FORWARD / DFFT_INVERSE: the direction whose dfft_get_pipeline_tables the step's exchange uses -- the
                             * chain's own, except in the chain of dfft_exec_spectral_op: forward up to its "xx" step, inverse from it on */
} dfft_chain_step;
/* the steps of the chain the next exec in `direction` (DFFT_SPECTRAL_OP with dims = 3: dfft_exec_spectral_op; DFFT_SPECTRAL_OPS with dims = 3:
 * dfft_exec_spectral_ops with as many outputs as option "spectral_outputs" says, empty while that is 1 -- fewer outputs run its first
 * 2 + 3 nout steps, and the step at position 2 + 3 j + {0, 1, 2} belongs to output j; DFFT_SPECTRAL_SUM with dims = 3:
 * dfft_exec_spectral_sum with as many inputs as option "spectral_inputs" says, empty while that is 1 -- the step at position
 * 3 j + {0, 1, 2} belongs to input j, and fewer inputs run the chain a plan with that option value has) of `dims` dimensions
 * (1, 2: exec_dim's partial transforms; 3: the whole transform) would run, as options read at exec time choose it; *count receives the number of steps, at most `capacity` are written */
int dfft_debug_get_chain(const dfft_plan *plan, int direction, int dims, dfft_chain_step *steps, int capacity, int *count);
/* One operation of the stream and event schedule of an exec (dfft_debug_trace_chain), in the order the exec issues them.  The executor
 * (run_chain, csrc/dfft.hip) has one loop that decides the schedule; its launches, exchanges, event records and stream waits go through
 * a sink that either issues them or only lists them, so this list is what an exec does, not a restatement of it.  Operations on one
 * stream run in the order issued; a wait orders its stream behind the latest record of that event issued before it.  Fields that do not
 * apply to a kind are -1 (which, scratch: 0). */
typedef struct dfft_trace_op {
    int32_t kind;           /* 0 launch, 1 exchange, 2 event record, 3 stream wait */
    int32_t stream;         /* 0 the plan's stream (dfft_set_stream), 1 second compute stream, 2 communication stream, 3 second
                             * communication stream */
    int32_t event;          /* record / wait: number of the event within this exec */
    int32_t step, chunk;    /* launch / exchange: index into dfft_debug_get_chain's steps, pipeline chunk */
    int32_t launch;         /* launch: index within its group (what dfft_debug_get_pass takes) */
    int32_t src, dst;       /* as in dfft_chain_step; exchange: send buffer, receive buffer */
    int32_t which;          /* exchange: 1 / 2 */
    int32_t scratch;        /* launch: 1 if it goes through the plan's shared level scratch (two-level and long-Bluestein lines) */
} dfft_trace_op;
/* dims = 1, 2, 3: the schedule the next exec in `direction` of `dims` dimensions would issue, as the options and the transport
 * stand now (host only; no device needed).  Whether the second compute stream and the communication streams are used is a predicate of
 * the plan -- option "compute_streams", the chain, the pipeline depth, the level scratch, option "graph", the transport's
 * concurrent channels -- that the exec evaluates in the same way; a stream it asks for is created when an exec first needs it.
 * dims = 0: what the last exec in `direction` (whole or partial) issued while option "trace" was 1; empty if there was none.  (A
 * replayed hipGraph, option "graph", issues nothing: the list stays that of the exec that was captured.)
 * *count receives the number of operations, at most `capacity` are written. */
int dfft_debug_trace_chain(const dfft_plan *plan, int direction, int dims, dfft_trace_op *ops, int capacity, int *count);
/* the per-point address table the kernels use for a segmented side of that launch (store = 0: load
 * side, 1: store side); entry i = {base[i], ln[i], aux[i]} as documented for SegEntry.  *count receives
 * the number of points; at most `capacity` entries are written. */
int dfft_debug_get_point_table(const dfft_plan *plan, const char *name, int index, int store, uint64_t *base,
                               uint32_t *ln, uint32_t *aux, size_t capacity, size_t *count);

const char *dfft_last_error(void);
const char *dfft_version(void);
/* kernel configuration for line length N: returns 0 if supported and fills the fields */
int dfft_kernel_info(int precision, size_t N, int *threads, int *lds_bytes, int *points_per_thread,
                     int *lines_per_workgroup);
/* how an axis of N points is transformed (the plan cufftMakePlanMany64 hides, mpicufft_pencil_opt1.cpp:165-197): returns 0 and fills
 * info[0] = 0 native chain / 1 Bluestein / 2 two levels (N = N1*N2 over two launches) / 3 long Bluestein (a length that neither fits
 * one launch nor splits, e.g. a prime above 4096: Bluestein's algorithm on info[1] padded points whose transforms are two-level lines;
 * four launches), info[1] = inner power-of-two length (0 for two levels), and for two levels / long Bluestein info[2..4] = {N1, its
 * inner length, 1 if Bluestein} and info[5..7] likewise for N2 (the levels of the padded length in the long form).
 * two_level = 1: two levels wherever N splits (the plan option of the same name).  ERR_UNSUPPORTED: no plan (beyond 2^23 points). */
int dfft_axis_plan_info(int precision, size_t N, int two_level, size_t info[8]);

/* ---- placement-aware device memory (no counterpart in the reference, whose buffers are plain cudaMalloc,
 * src/pencil/mpicufft_pencil_opt1.cpp:344-365; the analogue of fftw_malloc + FFTW_MEASURE) ----------------
 * The passes that write 128-byte runs (y, x) run 5-10 % faster or slower depending on the PHYSICAL backing of the
 * buffer they scatter to -- per buffer, for the life of the allocation (profiles/r3_placement.txt).
 * dfft_malloc: chunk_mib = 0 is hipMalloc; otherwise one virtual range backed by physical allocations of chunk_mib MiB
 * each (HIP virtual-memory API).  chunk_mib = DFFT_CHUNK_DEFAULT: the library's default backing, which is also what the library
 * uses for a work area it owns (dfft_init(allocate = 1), dfft_set_work_area(plan, NULL, NULL)): 1 GiB chunks (smaller ones and
 * finally hipMalloc if that fails) and, for buffers of 1 GiB and more, PLACEMENT.  Such a buffer is built from chunks that lie far
 * apart (every K-th of K times as many, K = 5 unless DFFT_PLACEMENT_SPREAD says otherwise or memory is short) and a streaming write is
 * timed on it (8 ms per 16 GiB): the good class by construction; the first one of a process gives the device its yardstick, and a
 * built buffer at >= 0.95 x the yardstick is kept.  Where there is no room for the pool, or the built buffer falls short,
 * plain candidates are drawn, up to DFFT_PLACEMENT_TRIES (6), all alive, and the fastest of everything probed is kept.  Nothing is absolute: the
 * yardstick is measured on the device at hand (MI355X: built buffers 6.5 - 7.0 TB/s, bad ones 5.2 - 5.8, a contiguous hipMalloc
 * reference 4.5 - 4.6; the plan's scatter passes follow: 5.5 vs 5.9 - 6.5 ms per pass at 1024^3 fp64, profiles/r4_placement_probe.txt,
 * profiles/r5_allocator.txt); DFFT_PLACEMENT_GOOD_TBPS sets an absolute threshold.  Everything alive during the search stays within
 * half of the free memory divided by DFFT_RANKS_PER_DEVICE (set it when several processes share a GPU), and whatever fails on the way
 * falls back to the plain recipe and then to hipMalloc: the call never fails where hipMalloc would succeed.  1024^3 fp64 forward +
 * inverse on buffers from this call: 33.5 - 33.6 ms, on hipMalloc buffers 37.0 - 38.3.  Local to the device (no plan, no collective):
 * safe on every rank of a multi-rank job.  Costs 2 - 4 s per 16 GiB buffer (the driver clears fresh memory inside hipMemCreate at
 * ~30 ms per GiB: tools/vmm_cycle), 0.3 s per 2 GiB; DFFT_PLACEMENT_SPREAD=1: milliseconds (plain candidates only, no yardstick).  Environment: DFFT_DEFAULT_CHUNK_MIB
 * (0 = hipMalloc), DFFT_PLACEMENT_TRIES (1 = no probe), DFFT_PLACEMENT_SPREAD, DFFT_RANKS_PER_DEVICE, DFFT_PLACEMENT_GOOD_TBPS.
 * Addresses: on this ROCm a virtual address that is mapped a SECOND time (after hipMemAddressFree and a later reservation at the
 * same address, or fresh chunks mapped into a kept reservation) reads and writes wrong bytes -- tools/vmm_reuse_repro.hip reproduces
 * it without this library, with kernels and with runtime copies, in 2 - 90 map / unmap cycles (profiles/r6_vmm_reuse_repro.txt) --
 * and a range that is unmapped but not freed keeps its physical memory (profiles/r6_vmm_cost.txt).  So dfft_free unmaps AND returns
 * the range, and dfft_malloc reserves every range at an address it names itself and never names twice: the library walks once
 * through [DFFT_VMM_BASE_TIB = 4 TiB, 80 TiB) of the process's address space (profiles/r6_vmm_hint.txt: 10^4 cycles, device memory
 * level, not one wrong byte).  When that region is used up the default backing is hipMalloc.
 * dfft_last_placement_info writes what the last placement-aware allocation of the process did (a JSON object: K, candidates drawn,
 * probe / reference / threshold rates, seconds by phase, what was kept).  Free with dfft_free (which also takes pointers it did not
 * allocate: hipFree; it synchronises the owning device first, like hipFree). */
#define DFFT_CHUNK_DEFAULT ((size_t)-1)
int dfft_malloc(size_t bytes, size_t chunk_mib, void **ptr);
int dfft_free(void *ptr);
int dfft_last_placement_info(char *buf, size_t capacity);
/* Tries up to `tries` backings for the plan's own work area (only when the library owns it), for a new output buffer
 * *out (dfft_domain_size bytes) and, if back != NULL, for a new buffer *back of the input block's size (the inverse
 * transform's output), one buffer at a time, and keeps for each the backing on which the plan's own FFT passes
 * (forward in -> out, inverse out -> back; exchanges not counted) run fastest.  `in` must hold a valid input block; it
 * is only read.  Afterwards the y / x passes try their streaming (nontemporal) kernel configuration on the chosen buffers and
 * keep it where it measures faster.  *out / *back are freed with dfft_free.  On a multi-rank plan the call is collective and
 * does NOT search (how many candidates fit is a per-rank matter: ranks running different numbers of trials would strand each
 * other in an exchange): out / back come from the default backing and only the configuration trials run, whose number depends
 * on the global grid alone.  report_ms (optional): the measured pass time of every trial in order, *n_report
 * entries. */
int dfft_tune_placement(dfft_plan *plan, const void *in, int tries, void **out, void **back, float *report_ms,
                        int max_report, int *n_report);
/* The second half of dfft_tune_placement on the caller's own buffers (no allocation).  First every pass tries the four
 * workgroup -> tile orders, then every kernel configuration its line length has (streaming siblings, other lane mappings and
 * tile shapes: the role variants of csrc/cfg_*.hip.h).  A trial sets all passes at once and reads the per-pass times from the
 * phase timers, so each pass picks for itself (1 % threshold) from 4 + (number of configuration numbers) trials; passes the
 * caller pinned with order_* / variant_* keep their setting, Bluestein / two-level axes and the slab sequences are not tuned.
 * A trial executes the plan three times forward in -> out and, if back != NULL, inverse out -> back, which destroys `out` like
 * every inverse.  Collective on a multi-rank plan: which trials run depends on the global grid only, every rank decides for its
 * own kernels.  report_ms: the plan as built, the four order settings, the chosen orders, one entry per configuration number,
 * the final choice. */
int dfft_tune_variants(dfft_plan *plan, const void *in, void *out, void *back, float *report_ms, int max_report, int *n_report);

#ifdef __cplusplus
}
#endif
#endif /* DFFT_C_H */
