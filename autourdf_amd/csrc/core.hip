// core.hip -- version, error string, device check.
#include <cstring>
#include "creg_common.h"

namespace creg {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace creg

extern "C" int creg_version(void) { return 2200; }  // 2200: creg_mesh_cover_f64 (the cloud fit's other direction: per posed triangle the nearest point and the number of points within d_max); 2100: creg_feature_moments_f64 (the link moments and the 21 sums of the matched feature's curvature: sum A^T Pi A per pose and link); 2000: creg_link_moments_f64 (16 moment sums per pose and link: the twist system of refining joint frames); 1900: creg_pose_fit_system_f64 (the Gauss-Newton system of fitting a URDF to clouds); 1700: creg_joint_types_f64 / creg_joint_slides_f64 (prismatic and fixed joints: the kind of every edge, slide positions); 1600: creg_lattice_hull_i32 / creg_lattice_hull_emit_i32 (exact convex collision hulls of the links); 1500: creg_link_poses_f64 / creg_joint_positions_f64 / creg_motion_error_f64 (joint positions, limits, the replay check); 1400: creg_mesh_contain_f64 (a link wholly inside another, winding numbers); 1300: creg_mesh_clearance_f64 (link clearance, the collision margin); 1200: creg_mesh_inertia_f64 (mass properties of link meshes); 1100: creg_mesh_collide_f64 (self-collision of posed link meshes); 1000: creg_raster_depth_f64 / creg_depth_points_f64 / creg_segment_plane_f64 (depth-camera frames, ground removal); 900: creg_urdf_fk_f64 (batched forward kinematics, evaluation stage); 800: creg_joint_axes_f64 / creg_link_clouds_f64 (joints, link clouds); 700: creg_link_sweep_f64 / creg_coord_mst_f64 (URDF stage); round 6: creg_train_plan_resume / creg_train_state, creg_train_plan_info_t.chain_probe_us, creg_icp_nn_counters (400: y_unchanged, named info fields)
extern "C" const char* creg_last_error(void) { return creg::g_err; }
extern "C" int creg_device_check(void) {
    int dev = 0;
    CREG_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    CREG_HIP(hipGetDeviceProperties(&p, dev));
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) {
        creg::set_error("libcreg is built for gfx950 only, current device is %s", p.gcnArchName);
        return CREG_EARCH;
    }
    return CREG_OK;
}
