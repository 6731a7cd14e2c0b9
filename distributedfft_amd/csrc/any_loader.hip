// any_loader.hip -- the core library's side of the second, lazily loaded library libdfft_amd_any.so.
//
// libdfft_amd.so holds the kernels of the power-of-two lengths 2 .. 8192 (complex axis passes and the packed real z passes): every
// BASELINE configuration, ~13 core-minutes to compile.  The kernels of every OTHER length -- the 49 mixed-radix lengths 2^a 3^b 5^c 7^d
// <= 2048, their packed real forms and fused spectral-operator passes, and the generic kernel (Bluestein passes, two-level lines, long Bluestein) -- are ~45 core-minutes
// of template instantiations that no BASELINE configuration touches (profiles/r6_cold_build_per_object.txt); they live in
// libdfft_amd_any.so next to this library (any_exports.hip), which is opened at the first plan that needs one of them.  The
// functions below are the entry points the rest of the core calls (kernels_*.hip, real_*.hip, dfft.hip: launch_generic); they forward
// through the C symbols of the second library, after dfft_any_abi has shown that it was built with this library's PassArgs and PassInfo.  There is no fallback: when it is missing, dfft_init of such a plan fails and says
// which file to build.
#include <dlfcn.h>
#include <stdlib.h>

#include <mutex>
#include <string>

#include "fft_pass.hip.h"
#include "dfft_internal.hpp"

namespace dfft {
namespace {
using launch3_fn = int (*)(int, int, const PassArgs *, hipStream_t);
using launch2_fn = int (*)(int, const PassArgs *, hipStream_t);
using info3_fn = int (*)(int, int, PassInfo *);
using info1_fn = int (*)(int);

struct AnyLib {
    void *handle = nullptr;
    std::string why;                       // why it is not available
    std::string spectral_why;              // why the fused spectral-operator passes are not (a library from before they existed)
    launch3_fn launch_mixed[2] = {nullptr, nullptr}, launch_rmixed[2] = {nullptr, nullptr};      // [0] f64, [1] f32
    info3_fn mixed_info[2] = {nullptr, nullptr};
    info1_fn rmixed_info[2] = {nullptr, nullptr};
    launch2_fn launch_bluestein[2] = {nullptr, nullptr};
    launch2_fn launch_spectral_mixed[2] = {nullptr, nullptr};
    info1_fn spectral_mixed_supported[2] = {nullptr, nullptr};
};
AnyLib g_any;
std::once_flag g_any_once;

void load_once()
{
    AnyLib &lib = g_any;
    std::string path;
    if (const char *e = getenv("DFFT_ANY_LIBRARY")) path = e;      // tests: another build, or a name that does not exist
    else {
        Dl_info di;
        if (!dladdr(reinterpret_cast<const void *>(&load_once), &di) || !di.dli_fname) { lib.why = "dladdr failed"; return; }
        path = di.dli_fname;
        const size_t slash = path.rfind('/');
        path = (slash == std::string::npos ? std::string() : path.substr(0, slash + 1)) + "libdfft_amd_any.so";
    }
    void *h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) {
        const char *de = dlerror();
        lib.why = "cannot load " + path + (de ? std::string(": ") + de : std::string()) + " -- build it with `make -C distributedfft_amd/csrc any` (or __graft_entry__.build())";
        return;
    }
    bool ok = true;
    auto sym = [&](const char *name) { void *s = dlsym(h, name); if (!s) { ok = false; lib.why = path + " lacks the symbol " + name; } return s; };
    lib.launch_mixed[0] = (launch3_fn)sym("dfft_any_launch_mixed_f64");   lib.launch_mixed[1] = (launch3_fn)sym("dfft_any_launch_mixed_f32");
    lib.mixed_info[0] = (info3_fn)sym("dfft_any_mixed_info_f64");         lib.mixed_info[1] = (info3_fn)sym("dfft_any_mixed_info_f32");
    lib.launch_rmixed[0] = (launch3_fn)sym("dfft_any_launch_rmixed_f64"); lib.launch_rmixed[1] = (launch3_fn)sym("dfft_any_launch_rmixed_f32");
    lib.rmixed_info[0] = (info1_fn)sym("dfft_any_rmixed_info_f64");       lib.rmixed_info[1] = (info1_fn)sym("dfft_any_rmixed_info_f32");
    lib.launch_bluestein[0] = (launch2_fn)sym("dfft_any_launch_bluestein_f64");
    lib.launch_bluestein[1] = (launch2_fn)sym("dfft_any_launch_bluestein_f32");
    // PassArgs and PassInfo cross the seam by pointer: a library built from another version of either struct is refused
    if (ok) {
        using abi_fn = void (*)(size_t[3]);
        const std::string rebuild = " -- rebuild it with `make -C distributedfft_amd/csrc any`";
        abi_fn abi = (abi_fn)dlsym(h, "dfft_any_abi");
        if (!abi) {
            ok = false;
            lib.why = path + " lacks the symbol dfft_any_abi (a build from before the check of the kernel argument structs)" + rebuild;
        } else {
            size_t theirs[3] = {0, 0, 0};
            const size_t mine[3] = {sizeof(PassArgs), sizeof(PassInfo), (size_t)DFFT_PASS_ABI};
            abi(theirs);
            if (theirs[0] != mine[0] || theirs[1] != mine[1] || theirs[2] != mine[2]) {
                auto list = [](const size_t v[3]) {
                    return "sizeof(PassArgs) " + std::to_string(v[0]) + ", sizeof(PassInfo) " + std::to_string(v[1]) + ", DFFT_PASS_ABI " + std::to_string(v[2]);
                };
                ok = false;
                lib.why = path + " was built for another version of the kernel argument structs (" + list(theirs) + "; this library: " + list(mine) + ")" + rebuild;
            }
        }
    }
    // the fused spectral-operator passes of the mixed-radix lengths came later than the rest: a library without them still serves every
    // other plan, and dfft_init of a plan that needs them (option spectral_op = 2) says what is missing
    if (ok) {
        const char *names[4] = {"dfft_any_launch_spectral_mixed_f64", "dfft_any_launch_spectral_mixed_f32",
                                "dfft_any_spectral_mixed_supported_f64", "dfft_any_spectral_mixed_supported_f32"};
        void *s[4];
        for (int i = 0; i < 4; i++)
            if (!(s[i] = dlsym(h, names[i])) && lib.spectral_why.empty())
                lib.spectral_why = path + " lacks the symbol " + names[i] + " -- rebuild it with `make -C distributedfft_amd/csrc any`";
        if (lib.spectral_why.empty()) {
            lib.launch_spectral_mixed[0] = (launch2_fn)s[0]; lib.launch_spectral_mixed[1] = (launch2_fn)s[1];
            lib.spectral_mixed_supported[0] = (info1_fn)s[2]; lib.spectral_mixed_supported[1] = (info1_fn)s[3];
        }
    }
    if (ok) lib.handle = h; else dlclose(h);
}
AnyLib *any()
{
    std::call_once(g_any_once, load_once);
    return g_any.handle ? &g_any : nullptr;
}
}  // namespace

// is libdfft_amd_any.so there?  (*why: the reason when it is not)
bool any_available(std::string *why)
{
    if (any()) return true;
    if (why) *why = g_any.why;
    return false;
}

// are the fused spectral-operator passes of the mixed-radix lengths there?  (*why: the reason when they are not)
bool any_spectral_mixed_available(std::string *why)
{
    AnyLib *l = any();
    if (l && l->spectral_why.empty()) return true;
    if (why) *why = l ? l->spectral_why : g_any.why;
    return false;
}

// "no kernel for this length" (-1 / false) when the library is missing, exactly like a length without a configuration: the plan
// then looks for another form of the axis, ends at the generic kernel, and dfft_init reports why that is not available either
int launch_mixed_f64(int N, int variant, const PassArgs &A, hipStream_t s) { AnyLib *l = any(); return l ? l->launch_mixed[0](N, variant, &A, s) : -1; }
int launch_mixed_f32(int N, int variant, const PassArgs &A, hipStream_t s) { AnyLib *l = any(); return l ? l->launch_mixed[1](N, variant, &A, s) : -1; }
bool mixed_info_f64(int N, int variant, PassInfo *pi) { AnyLib *l = any(); return l && l->mixed_info[0](N, variant, pi) != 0; }
bool mixed_info_f32(int N, int variant, PassInfo *pi) { AnyLib *l = any(); return l && l->mixed_info[1](N, variant, pi) != 0; }
int launch_rmixed_f64(int M, int mode, const PassArgs &A, hipStream_t s) { AnyLib *l = any(); return l ? l->launch_rmixed[0](M, mode, &A, s) : -1; }
int launch_rmixed_f32(int M, int mode, const PassArgs &A, hipStream_t s) { AnyLib *l = any(); return l ? l->launch_rmixed[1](M, mode, &A, s) : -1; }
bool rmixed_info_f64(int M) { AnyLib *l = any(); return l && l->rmixed_info[0](M) != 0; }
bool rmixed_info_f32(int M) { AnyLib *l = any(); return l && l->rmixed_info[1](M) != 0; }
int launch_bluestein_f64(int M, const PassArgs &A, hipStream_t s) { AnyLib *l = any(); return l ? l->launch_bluestein[0](M, &A, s) : -1; }
int launch_bluestein_f32(int M, const PassArgs &A, hipStream_t s) { AnyLib *l = any(); return l ? l->launch_bluestein[1](M, &A, s) : -1; }
int launch_spectral_mixed_f64(int N, const PassArgs &A, hipStream_t s) { AnyLib *l = any(); return l && l->launch_spectral_mixed[0] ? l->launch_spectral_mixed[0](N, &A, s) : -1; }
int launch_spectral_mixed_f32(int N, const PassArgs &A, hipStream_t s) { AnyLib *l = any(); return l && l->launch_spectral_mixed[1] ? l->launch_spectral_mixed[1](N, &A, s) : -1; }
bool spectral_mixed_supported_f64(int N) { AnyLib *l = any(); return l && l->spectral_mixed_supported[0] && l->spectral_mixed_supported[0](N) != 0; }
bool spectral_mixed_supported_f32(int N) { AnyLib *l = any(); return l && l->spectral_mixed_supported[1] && l->spectral_mixed_supported[1](N) != 0; }
}  // namespace dfft
