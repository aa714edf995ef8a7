// hand_check.h -- host-side argument checks of the entries that take a hand model as a pn2x_hand_pose_setup record
// (hand_pose.hip, hand_interact.hip): one precedence of the error codes and one statement of what a usable model is.
#pragma once
#include <cstdint>

#include "../../include/pn2_ext.h"

namespace pn2 {

// What an entry's argument checks found, whichever check found it: a bad value before a limit before a NULL pointer.
struct Faults {
    bool inval = false, range = false, null = false;
    int code() const { return inval ? PN2_EINVAL : range ? PN2_ERANGE : null ? PN2_ENULL : PN2_OK; }
};

// A record pointer is read only if a process can own the address: nothing is mapped below 64 KiB.  A caller built against
// ABI version 3 passes its candidate count where the setup record is now, and is refused (PN2_EINVAL) instead of read.
inline bool is_record(const void *rec) { return (uintptr_t)rec >= 65536; }
inline bool is_record(const void *rec, Faults &f) {
    if (is_record(rec)) return true;
    (rec ? f.inval : f.null) = true;
    return false;
}

// the model in a readable setup record: what every entry reads of it (the range check is the entry's: it knows its p)
inline void check_hand_model(const pn2x_hand_pose_setup &s, Faults &f) {
    f.inval |= s.v < 1 || s.j < 1 || s.k < 1 || s.res < 1 || (s.res & 1) == 0 || !(s.voxel_scale > 0.f) ||
               (s.vol_f16 != 0 && s.vol_f16 != 1);
    f.null |= !s.parents || !s.pose_block || !s.skin_pack || !s.skin_w;
    if (s.posedirs) {  // the MANO part; posedirs is read by 16-byte loads
        f.inval |= (s.centre_root != 0 && s.centre_root != 1) || ((uintptr_t)s.posedirs & 15);
        f.null |= !s.pose_mean || !s.kp_vertex;
    }
}

}  // namespace pn2
