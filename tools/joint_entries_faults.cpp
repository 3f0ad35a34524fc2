// Stand-alone check of the joint entries' argument handling, for a host-side sanitizer build: every call below has one bad
// argument (or J == 0) and returns before any HIP call, so it runs without a GPU.  The pointers are made-up addresses
// that are never dereferenced.  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-omit-frame-pointer tools/joint_entries_faults.cpp autourdf_amd/csrc/core.hip \
//       autourdf_amd/csrc/joints.hip autourdf_amd/csrc/joint_types.hip autourdf_amd/csrc/joint_motion.hip -o joint_entries_faults
//   ./joint_entries_faults
//
// tests/test_joint_entries_cpu.py pins the same calls' texts through ctypes; here they only have to say CREG_EINVAL
// with the entry's name in front, and the sanitizers have to stay silent.
#include <cmath>
#include <cstdio>
#include <cstring>
#include "../include/creg.h"

static int failures = 0;

static void expect(int rc, int want, const char* who, const char* what) {
    const char* text = creg_last_error();
    const bool ok = rc == want && (want == CREG_OK || std::strncmp(text, who, std::strlen(who)) == 0);
    if (!ok) ++failures;
    std::printf("%s %-26s %-22s rc %d  %s\n", ok ? "ok  " : "FAIL", who, what, rc, want == CREG_OK ? "" : text);
}

int main() {
    double* d = reinterpret_cast<double*>(0x1000);
    int32_t* i = reinterpret_cast<int32_t*>(0x2000);
    auto axes = [&](const double* coords, int S, int T, int K, int J, int start, int num, int interval, double* sample) {
        return creg_joint_axes_f64(coords, S, T, K, i, i, 8, i, J, start, num, interval, sample, d, d, i, d, d, d, d, i, d, nullptr);
    };
    auto types = [&](const double* coords, int S, int T, int K, int J, int start, int num, int interval, double turn, double slide) {
        return creg_joint_types_f64(coords, S, T, K, i, i, 8, 4, i, J, start, num, interval, turn, slide, d, d, i, i, i, d, d, d, nullptr);
    };
    auto positions = [&](const double* link_T, int S, int J, int ref_seq, int ref_step, int start, int num) {
        return creg_joint_positions_f64(link_T, S, 20, 4, i, J, d, d, ref_seq, ref_step, start, num, d, d, d, d, i, nullptr);
    };
    auto slides = [&](const double* link_T, int S, int J, int ref_seq, int ref_step, int start, int num) {
        return creg_joint_slides_f64(link_T, S, 20, 4, i, J, d, ref_seq, ref_step, start, num, d, d, d, d, i, nullptr);
    };
    const char *A = "creg_joint_axes_f64", *Ty = "creg_joint_types_f64", *P = "creg_joint_positions_f64", *Sl = "creg_joint_slides_f64";
    expect(axes(d, 2, 20, 257, 3, 0, 10, 1, d), CREG_EINVAL, A, "K = 257");
    expect(axes(d, 2, 20, 8, 3, 0, 0, 1, d), CREG_EINVAL, A, "num_steps = 0");
    expect(axes(d, 2, 20, 8, 3, 0, 10, 0, d), CREG_EINVAL, A, "interval = 0");
    expect(axes(d, 2, 20, 8, 3, 11, 10, 1, d), CREG_EINVAL, A, "a step past T");
    expect(axes(d, 1, 5000, 8, 3, 0, 4098, 1, d), CREG_EINVAL, A, "4097 samples");
    expect(axes(nullptr, 2, 20, 8, 3, 0, 10, 1, d), CREG_EINVAL, A, "null coords");
    expect(axes(d, 2, 20, 8, 3, 0, 10, 1, nullptr), CREG_EINVAL, A, "null sample output");
    expect(axes(d, 2, 20, 8, 0, 0, 10, 1, d), CREG_OK, A, "J = 0");
    expect(types(d, 2, 20, 257, 3, 0, 10, 1, 2e-4, 1e-6), CREG_EINVAL, Ty, "K = 257");
    expect(types(d, 2, 20, 8, 3, 0, 0, 1, 2e-4, 1e-6), CREG_EINVAL, Ty, "num_steps = 0");
    expect(types(d, 2, 20, 8, 3, 0, 10, 0, 2e-4, 1e-6), CREG_EINVAL, Ty, "interval = 0");
    expect(types(d, 2, 20, 8, 3, 11, 10, 1, 2e-4, 1e-6), CREG_EINVAL, Ty, "a step past T");
    expect(types(d, 1, 5000, 8, 3, 0, 4098, 1, 2e-4, 1e-6), CREG_EINVAL, Ty, "4097 samples");
    expect(types(nullptr, 2, 20, 8, 3, 0, 10, 1, 2e-4, 1e-6), CREG_EINVAL, Ty, "null coords");
    expect(types(d, 2, 20, 8, 3, 0, 10, 1, NAN, 1e-6), CREG_EINVAL, Ty, "turn_min = nan");
    expect(types(d, 2, 20, 8, 3, 0, 10, 1, 2e-4, INFINITY), CREG_EINVAL, Ty, "slide_min = inf");
    expect(types(d, 2, 20, 8, 3, 0, 10, 1, -1e-3, 1e-6), CREG_EINVAL, Ty, "turn_min < 0");
    expect(types(d, 2, 20, 8, 3, 0, 10, 1, 2e-4, -1.0), CREG_EINVAL, Ty, "slide_min < 0");
    expect(types(nullptr, 2, 20, 8, 0, 0, 10, 1, 2e-4, 1e-6), CREG_OK, Ty, "J = 0, null coords");
    expect(positions(d, 2, 3, 0, 0, 0, 0), CREG_EINVAL, P, "num_steps = 0");
    expect(positions(d, 2, 3, 0, 0, 11, 10), CREG_EINVAL, P, "a step past T");
    expect(positions(d, 65536, 3, 0, 0, 0, 10), CREG_EINVAL, P, "S = 65536");
    expect(positions(d, 2, 3, 2, 0, 0, 10), CREG_EINVAL, P, "ref_seq = S");
    expect(positions(d, 2, 3, 0, 20, 0, 10), CREG_EINVAL, P, "ref_step = T");
    expect(positions(nullptr, 2, 3, 0, 0, 0, 10), CREG_EINVAL, P, "null link_T");
    expect(positions(nullptr, 2, 0, 0, 0, 0, 10), CREG_OK, P, "J = 0, null link_T");
    expect(slides(d, 2, 3, 0, 0, 0, 0), CREG_EINVAL, Sl, "num_steps = 0");
    expect(slides(d, 2, 3, 0, 0, 11, 10), CREG_EINVAL, Sl, "a step past T");
    expect(slides(d, 65536, 3, 0, 0, 0, 10), CREG_EINVAL, Sl, "S = 65536");
    expect(slides(d, 2, 3, 2, 0, 0, 10), CREG_EINVAL, Sl, "ref_seq = S");
    expect(slides(d, 2, 3, 0, 20, 0, 10), CREG_EINVAL, Sl, "ref_step = T");
    expect(slides(nullptr, 2, 3, 0, 0, 0, 10), CREG_EINVAL, Sl, "null link_T");
    expect(slides(nullptr, 2, 0, 0, 0, 0, 10), CREG_OK, Sl, "J = 0, null link_T");
    std::printf("%d failure(s)\n", failures);
    return failures != 0;
}
