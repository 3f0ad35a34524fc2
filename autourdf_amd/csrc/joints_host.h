// joints_host.h -- host side of the joint entries: the argument checks creg_joint_axes_f64 (joints.hip) and
// creg_joint_types_f64 (joint_types.hip) share, written once.  The limits are joints_dev.h's.
#pragma once
#include "creg_common.h"
#include "joints_dev.h"

namespace creg {

// Sizes, steps and the sample count of an entry that works on creg_joint_axes_samples' samples.  `L` is null for an
// entry without a link count.  Returns NS, or -1 with the error set under the entry's own name `who`.
static inline int joint_sample_count(const char* who, int32_t S, int32_t T, int32_t K, const int32_t* L, int32_t J,
                                     int32_t n_link_clusters, int32_t start_step, int32_t num_steps, int32_t interval) {
    if (!(S >= 1 && T >= 1 && K >= 1 && K <= JOINT_MAX_K && J >= 0 && (!L || *L >= 1) && n_link_clusters >= 1)) {
        if (L) set_error("%s: bad size (S=%d, T=%d, K=%d, L=%d, J=%d; K <= %d)", who, S, T, K, *L, J, JOINT_MAX_K);
        else set_error("%s: bad size (S=%d, T=%d, K=%d, J=%d; K <= %d)", who, S, T, K, J, JOINT_MAX_K);
        return -1;
    }
    if (!(start_step >= 0 && num_steps >= 1 && interval >= 1)) {
        set_error("%s: bad steps (start=%d, num=%d, interval=%d)", who, start_step, num_steps, interval);
        return -1;
    }
    if ((int64_t)start_step + num_steps > T) {
        set_error("%s: step %lld out of range for T=%d", who, (long long)start_step + num_steps - 1, T);
        return -1;
    }
    const int NS = creg_joint_axes_samples(S, num_steps, interval);
    if (NS > JOINT_MAX_SAMPLES) {
        set_error("%s: %d samples per joint (max %d)", who, NS, JOINT_MAX_SAMPLES);
        return -1;
    }
    return NS;
}

}  // namespace creg
