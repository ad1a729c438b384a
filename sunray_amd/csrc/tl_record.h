// The instance record of the two-level form: the one definition of its arithmetic, for the host loop (api.cpp two_level_build)
// and the device kernel (bvh_gpu.hip tl_records_kernel). Both sides are compiled with -ffp-contract=off, every operation is an
// IEEE one and none depends on a library's rounding, so both write the same bytes and the padding proof of DESIGN.md section 3
// is a proof about this function.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace srd {

enum TlRecordResult {
    kTlRecordOk = 0,
    kTlRecordNoFiniteBox = 1,    // w2o, pad_a, pad_b and the box are written; the box holds a non-finite value
    kTlRecordBaked = 2,          // the transform cannot be inverted (well): only w2o is written
};

__host__ __device__ inline double tl_max_d(double a, double b) { return a < b ? b : a; }   // std::max
__host__ __device__ inline double tl_min_d(double a, double b) { return b < a ? b : a; }   // std::min

// o2w: the 3 x 4 object-to-world transform; mesh_lo / mesh_hi: the (already padded) root box of the mesh's tree in object space;
// max_abs_vertex, max_edge_sum: the mesh's padding numbers; max_condition: ||W2O||_inf * ||O2W||_inf from which an instance is baked.
__host__ __device__ inline TlRecordResult tl_record(const float* o2w, const float* mesh_lo, const float* mesh_hi, float max_abs_vertex, float max_edge_sum,
                                                    double max_condition, float* w2o, float* lo_out, float* hi_out, float* pad_a, float* pad_b) {
    using std::isfinite;                         // the host's overloads next to the device's
    const float* M = o2w;
    const double eps = 5.9604644775390625e-08;   // 2^-24
    // inverse of the affine transform, in double
    const double a00 = M[0], a01 = M[1], a02 = M[2], a10 = M[4], a11 = M[5], a12 = M[6], a20 = M[8], a21 = M[9], a22 = M[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    const double id = 1.0 / det;
    const double R[9] = {c00 * id, (a02 * a21 - a01 * a22) * id, (a01 * a12 - a02 * a11) * id,
                         c01 * id, (a00 * a22 - a02 * a20) * id, (a02 * a10 - a00 * a12) * id,
                         c02 * id, (a01 * a20 - a00 * a21) * id, (a00 * a11 - a01 * a10) * id};
    const double T[3] = {M[3], M[7], M[11]};
    double r_norm = 0.0, m_norm = 0.0, t_max = 0.0;
    bool finite = isfinite(id) && det != 0.0;
    for (int row = 0; row < 3; row++) {
        for (int c = 0; c < 3; c++) w2o[4 * row + c] = (float)R[3 * row + c];
        w2o[4 * row + 3] = (float)(-(R[3 * row] * T[0] + R[3 * row + 1] * T[1] + R[3 * row + 2] * T[2]));
        r_norm = tl_max_d(r_norm, fabs(R[3 * row]) + fabs(R[3 * row + 1]) + fabs(R[3 * row + 2]));
        m_norm = tl_max_d(m_norm, fabs((double)M[4 * row]) + fabs((double)M[4 * row + 1]) + fabs((double)M[4 * row + 2]));
        t_max = tl_max_d(t_max, fabs(T[row]));
        for (int c = 0; c < 4; c++) finite = finite && isfinite(w2o[4 * row + c]);
    }
    // A transform of rank 2 still yields real (flat) world-space triangles, and a badly conditioned one stretches object space
    // against world space: whatever the fp32 triangle test's own rounding moves a hit by in world space (on sliver triangles
    // that is far more than a box's padding: the round-3 fuzzer found hits 8e-3 off their triangle) is multiplied by
    // ||W2O|| on the way into the mesh's boxes. Such an instance gets a private world-space copy of its mesh's tree and is walked
    // without a ray transform: there the boxes see exactly what the one-level form's boxes see.
    if (!finite || !(r_norm * m_norm < max_condition)) return kTlRecordBaked;
    // world box: the 8 corners of the mesh's (already padded) box, then padding for the rounding of the transformed vertices
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, p_max = 0.0;
    for (int corner = 0; corner < 8; corner++) {
        const double x = (corner & 1) ? mesh_hi[0] : mesh_lo[0], y = (corner & 2) ? mesh_hi[1] : mesh_lo[1], z = (corner & 4) ? mesh_hi[2] : mesh_lo[2];
        for (int row = 0; row < 3; row++) {
            const double w = (double)M[4 * row] * x + (double)M[4 * row + 1] * y + (double)M[4 * row + 2] * z + (double)M[4 * row + 3];
            lo[row] = tl_min_d(lo[row], w); hi[row] = tl_max_d(hi[row], w);
            p_max = tl_max_d(p_max, fabs(w));
        }
    }
    const double pad_w = 64.0 * eps * (p_max + m_norm * max_abs_vertex + t_max) + 8e-6 * m_norm * max_edge_sum;
    bool box_ok = true;
    for (int a = 0; a < 3; a++) {
        lo_out[a] = nextafterf((float)(lo[a] - pad_w), -INFINITY); hi_out[a] = nextafterf((float)(hi[a] + pad_w), INFINITY);
        box_ok = box_ok && isfinite(lo_out[a]) && isfinite(hi_out[a]);
    }
    // widening of the mesh's object-space boxes: rounding of the ray transform (grows with the ray origin) and of the world-space
    // vertices, plus the barycentric slack of the world-space triangle test seen from object space
    *pad_a = (float)(64.0 * eps * r_norm);
    *pad_b = (float)(r_norm * (64.0 * eps * (p_max + t_max + m_norm * max_abs_vertex) + 8e-6 * m_norm * max_edge_sum));
    return box_ok ? kTlRecordOk : kTlRecordNoFiniteBox;
}

}  // namespace srd
