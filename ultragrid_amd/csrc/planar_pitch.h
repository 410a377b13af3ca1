// planar_pitch.h -- the pitch rule of the planar shuffles (pixfmt.hip: ug_hip_uyvy_to_i420; planar.hip; planar_api.hip), stated in
// include/ug_mi355x.h: a pitch shorter than the bytes of a line the conversion reads or writes there is refused before any device call
#pragma once

#include "ug_common.h"

namespace ug {

/// (pitch, bytes of a line the conversion reads or writes there) pairs: a pitch shorter than its line folds lines onto each other and
/// carries the last one past the pitch * rows bytes the caller described
static inline bool lines_fit(std::initializer_list<long long> pitch_need)
{
        for (const long long *p = pitch_need.begin(); p + 1 < pitch_need.end(); p += 2) if (p[0] < p[1]) return false;
        return true;
}
static inline int refuse_short_pitch(const char *who)
{
        char msg[160];
        snprintf(msg, sizeof msg, "%s: a pitch is shorter than the line it holds", who);
        set_last_error_msg(msg);
        return UG_HIP_EINVAL;
}

} // namespace ug
