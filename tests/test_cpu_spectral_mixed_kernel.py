"""The register hand-off of fft_spectral_kernel (csrc/fft_pass.hip.h) for the mixed-radix x lengths of option spectral_op = 2, without a GPU:
tests/cpp/spectral_mixed_chain_check.hip drives the kernel's own building blocks on the host -- forward chain, the hand-off into register
spectral_sigma(c), second chain, conjugation, the store's index map -- for every configuration of the list macros of csrc/spectral_mixed.inc
(the ones the launchers of spectral_mixed_<p>.hip switch over, dedicated configurations included), against N * ifft(fft(x) * m) in long double.
Six forms per configuration: the array multiplier, the two real-table forms, and the factor forms (mkind 3, 4, 5) through the kernel's
spectral_factor_point / spectral_factor_line.  The hand-off walks the registers in the kernel's own chunks (spectral_chunk<Cfg>()) into
registers that start as NaN: with the chunk width the powers of two had, 4, the configurations with E = 10, 18, 30, 50 fail here.  The number of configurations checked is held to the number of mixed-radix lengths
dfft.spectral_op_supported reports: a length the library accepts and the emulation never saw cannot pass.
The translation unit is compiled in parts, all at once (host side only; about a minute of wall time on eight cores for both precisions)."""
import re

import distributedfft_amd as dfft

import host_check

PARTS = 4


def test_mixed_radix_chain_emulated_on_the_host(tmp_path):
    variants = [(f"{prec}_{k}", [*flag, f"-DCHECK_PARTS={PARTS}", f"-DCHECK_PART={k}"])
                for prec, flag in (("double", []), ("float", ["-DCHAIN_F32"])) for k in range(PARTS)]
    outputs = host_check.run(tmp_path, "spectral_mixed_chain_check.hip", variants, [*host_check.FLAGS, "--cuda-host-only"])
    counted = {"double": 0, "float": 0}
    for tag, out in outputs.items():
        m = re.search(r"(\d+) forms of (\d+) configurations checked, (\d+) failed", out)
        assert m and "ALL OK" in out, out[-2000:]
        assert int(m.group(1)) == 6 * int(m.group(2)) and int(m.group(3)) == 0, out[-2000:]
        counted[tag.split("_")[0]] += int(m.group(2))
    for prec in counted:
        mixed = [n for n in range(2, 2049) if n & (n - 1) and dfft.spectral_op_supported(n, prec, 2)]
        assert counted[prec] == len(mixed) > 40, (prec, counted[prec], mixed)
