// spectral_mixed.inc -- the mixed-radix x lengths of the fused forward-multiply-inverse pass (fft_spectral_kernel, option spectral_op = 2).
// Included inside namespace dfft behind kernels_mixed.inc, with DFFT_MIXED_F64 / DFFT_MIXED_F32 defined.  One list macro per precision,
// DFFT_<P>_SPECTRAL_MIXED(X) with X(N, 0, cfg), is the single source of the launcher switches and the "supported" predicates
// (spectral_mixed_<p>.hip) and of the host emulation (tests/cpp/spectral_mixed_chain_check.hip); the numbered shares are its compile parts
// (those of kernels_mixed.inc's axis-pass lists).
// A length is listed when all three instantiations (array, real tables, factor tables) compile without scratch
// (profiles/spectral_mixed_resources.txt).  F<P>_S<N> is a configuration for this kernel alone, where the axis pass's own (F<P>_M<N>) spills
// here or has sub-tile workgroups: same N, tile lines and G, SUB = 1, MAP = 0, at most 1024 threads, and at G = 1 an E that is not smaller (no more
// threads per line: the range check of dfft_exec_spectral_op counts with the axis pass's; spectral_mixed.hip.inc asserts all of it).  The
// twiddle table depends on N alone.
// Left out (dfft_init: ERR_UNSUPPORTED): fp32 1920 and fp32 2000 -- no configuration found without scratch (1920: E = 60 over four passes,
// 184 .. 364 B/lane for 30.4.4.4 and 20.12.4.2; 2000: 800 threads at E = 40 leave 128 VGPRs, 576 .. 640 B/lane, E = 50 and 80 are worse).
#ifdef DFFT_MIXED_F64
using F64_S2000 = PassCfg<double, 2000, 40, 8, 1, 20, 10, 10, 1, 1, 1>;   // 400 threads (F64_M2000, E = 20 and 800 threads: 12 B/lane with the factor tables)
#define DFFT_F64_SPECTRAL_MIXED0(X) X(12, 0, F64_M12) X(24, 0, F64_M24) X(36, 0, F64_M36) X(48, 0, F64_M48) X(72, 0, F64_M72) X(80, 0, F64_M80) X(120, 0, F64_M120) X(160, 0, F64_M160) X(192, 0, F64_M192) X(200, 0, F64_M200) X(240, 0, F64_M240) X(300, 0, F64_M300) X(384, 0, F64_M384) X(448, 0, F64_M448) X(500, 0, F64_M500) X(576, 0, F64_M576) X(600, 0, F64_M600) X(1000, 0, F64_M1000) X(1152, 0, F64_M1152) X(1200, 0, F64_M1200) X(1728, 0, F64_M1728) X(2000, 0, F64_S2000)
#define DFFT_F64_SPECTRAL_MIXED1(X) X(6, 0, F64_M6) X(10, 0, F64_M10) X(20, 0, F64_M20) X(40, 0, F64_M40) X(60, 0, F64_M60) X(96, 0, F64_M96) X(100, 0, F64_M100) X(112, 0, F64_M112) X(144, 0, F64_M144) X(224, 0, F64_M224) X(250, 0, F64_M250) X(288, 0, F64_M288) X(320, 0, F64_M320) X(400, 0, F64_M400) X(640, 0, F64_M640) X(720, 0, F64_M720) X(768, 0, F64_M768) X(800, 0, F64_M800) X(896, 0, F64_M896) X(1280, 0, F64_M1280) X(1536, 0, F64_M1536) X(1600, 0, F64_M1600) X(1792, 0, F64_M1792)
#define DFFT_F64_SPECTRAL_MIXED(X) DFFT_F64_SPECTRAL_MIXED0(X) DFFT_F64_SPECTRAL_MIXED1(X)
#define DFFT_F64_SPECTRAL_MIXED_FOREACH_SHARE(P) P(0) P(1)
#endif
#ifdef DFFT_MIXED_F32
using F32_S384 = PassCfg<float, 384, 24, 16, 2, 24, 4, 4, 1, 1, 1>;       // 512 threads (F32_M384, E = 48: 228 .. 376 B/lane)
using F32_S480 = PassCfg<float, 480, 60, 16, 2, 12, 10, 4, 1, 1, 1>;      // 256 threads (F32_M480, 30.4.4: 220 .. 236 B/lane)
using F32_S1200 = PassCfg<float, 1200, 60, 16, 1, 30, 10, 4, 1, 1, 1>;    // 320 threads (F32_M1200, E = 30 and 640 threads: 284 .. 296 B/lane)
using F32_S1600 = PassCfg<float, 1600, 40, 16, 1, 20, 20, 4, 1, 1, 1>;    // 640 threads (F32_M1600, 20.10.8: 12 B/lane)
#define DFFT_F32_SPECTRAL_MIXED0(X) X(6, 0, F32_M6) X(10, 0, F32_M10) X(36, 0, F32_M36) X(48, 0, F32_M48) X(96, 0, F32_M96) X(160, 0, F32_M160) X(224, 0, F32_M224) X(250, 0, F32_M250) X(500, 0, F32_M500) X(576, 0, F32_M576) X(1200, 0, F32_S1200) X(1536, 0, F32_M1536)
#define DFFT_F32_SPECTRAL_MIXED1(X) X(20, 0, F32_M20) X(40, 0, F32_M40) X(60, 0, F32_M60) X(144, 0, F32_M144) X(200, 0, F32_M200) X(320, 0, F32_M320) X(384, 0, F32_S384) X(480, 0, F32_S480) X(600, 0, F32_M600) X(896, 0, F32_M896) X(1000, 0, F32_M1000) X(1280, 0, F32_M1280)
#define DFFT_F32_SPECTRAL_MIXED2(X) X(12, 0, F32_M12) X(80, 0, F32_M80) X(112, 0, F32_M112) X(192, 0, F32_M192) X(400, 0, F32_M400) X(448, 0, F32_M448) X(960, 0, F32_M960) X(1152, 0, F32_M1152) X(1600, 0, F32_S1600) X(1728, 0, F32_M1728) X(1792, 0, F32_M1792)
#define DFFT_F32_SPECTRAL_MIXED3(X) X(24, 0, F32_M24) X(72, 0, F32_M72) X(100, 0, F32_M100) X(120, 0, F32_M120) X(240, 0, F32_M240) X(288, 0, F32_M288) X(300, 0, F32_M300) X(640, 0, F32_M640) X(720, 0, F32_M720) X(768, 0, F32_M768) X(800, 0, F32_M800) X(1440, 0, F32_M1440)
#define DFFT_F32_SPECTRAL_MIXED(X) DFFT_F32_SPECTRAL_MIXED0(X) DFFT_F32_SPECTRAL_MIXED1(X) DFFT_F32_SPECTRAL_MIXED2(X) DFFT_F32_SPECTRAL_MIXED3(X)
#define DFFT_F32_SPECTRAL_MIXED_FOREACH_SHARE(P) P(0) P(1) P(2) P(3)
#endif
