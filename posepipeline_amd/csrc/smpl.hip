// The SMPL body model on the device (smplx `lbs` with pose2rot = False), SPIN's 49-joint set, VIBE's weak-perspective projection and
// the rotation matrix -> axis-angle conversion: steps 5 - 8 of wrappers/vibe.py's network (posepipe_hip.h has the formulas).
//
// Six launches per call, all on the context's stream, every sum in a fixed order (fmaf chains; the sums over the V vertices are a
// per-thread chain over v = tid, tid + 256, ... followed by a fixed tree in LDS) -- no atomics, bit-identical from run to run:
//   smpl_shape_kernel    v_shaped = v_template + shapedirs . betas                       one thread per coordinate
//   smpl_regress_kernel  J = J_regressor . v_shaped  (and J_regressor_extra . verts)      one workgroup per (frame, joint)
//   smpl_pose_kernel     v_posed = v_shaped + pose_feature . posedirs                     one thread per coordinate, feature in LDS
//   smpl_chain_kernel    the 24-step rigid chain, one wave per frame                      lanes 0..11 = the 3 x 4 entries
//   smpl_skin_kernel     verts = (sum_i w_vi A_i) [v_posed; 1]                            one thread per vertex, A in LDS
//   smpl_joints_kernel   gather, re-index, project, axis-angle                            one wave per frame
// The mesh is small (6890 vertices, 83 KB per frame): every kernel is latency- or bandwidth-bound on posedirs (5.7 MB, read once
// per frame from the last-level cache).  Nothing about their speed is claimed beyond what tools/vibe_timing.py prints.
#include <cmath>

#include "pp_internal.h"

namespace {

constexpr int NJ = 24, NB = 10, NPF = 207, NPICK = 21, NEXTRA = 9, NJ54 = NJ + NPICK + NEXTRA, NOUT = 49;
__constant__ int c_parents[NJ] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};

__global__ __launch_bounds__(256) void smpl_shape_kernel(const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                                                         const float* __restrict__ betas, float* __restrict__ v_shaped, int V3) {
    const int f = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V3) return;
    const float* sd = shapedirs + (size_t)i * NB;
    const float* b = betas + (size_t)f * NB;
    float acc = 0.f;
#pragma unroll
    for (int l = 0; l < NB; ++l) acc = fmaf(sd[l], b[l], acc);
    v_shaped[(size_t)f * V3 + i] = v_template[i] + acc;
}

// out[f][r][c] = sum_v reg[r][v] pts[f][v][c];  grid (R, F), 256 threads
__global__ __launch_bounds__(256) void smpl_regress_kernel(const float* __restrict__ reg, const float* __restrict__ pts,
                                                           float* __restrict__ out, int V, int R) {
    __shared__ float red[3][256];
    const int r = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const float* w = reg + (size_t)r * V;
    const float* p = pts + (size_t)f * V * 3;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int v = tid; v < V; v += 256) {
        const float wv = w[v];
        a0 = fmaf(wv, p[3 * v + 0], a0);
        a1 = fmaf(wv, p[3 * v + 1], a1);
        a2 = fmaf(wv, p[3 * v + 2], a2);
    }
    red[0][tid] = a0; red[1][tid] = a1; red[2][tid] = a2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
            red[2][tid] += red[2][tid + s];
        }
        __syncthreads();
    }
    if (tid < 3) out[((size_t)f * R + r) * 3 + tid] = red[tid][0];
}

__global__ __launch_bounds__(256) void smpl_pose_kernel(const float* __restrict__ posedirs, const float* __restrict__ rotmat,
                                                        const float* __restrict__ v_shaped, float* __restrict__ v_posed, int V3) {
    __shared__ float pf[NPF];
    const int f = blockIdx.y;
    for (int k = threadIdx.x; k < NPF; k += 256) {
        const int e = k % 9;
        pf[k] = rotmat[(size_t)f * NJ * 9 + 9 + k] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V3) return;
    float acc = 0.f;
    for (int k = 0; k < NPF; ++k) acc = fmaf(pf[k], posedirs[(size_t)k * V3 + i], acc);
    v_posed[(size_t)f * V3 + i] = v_shaped[(size_t)f * V3 + i] + acc;
}

// one wave per frame.  G_i [3][4] in LDS; lanes 0..11 compute entry (r, c) of G_i = G_parent [R_i | J_i - J_parent].
// A [F][24][12] = G_i with G_i[:, :3] J_i taken off the translation; jt [F][24][3] = the chain translations (posed joints)
__global__ __launch_bounds__(64) void smpl_chain_kernel(const float* __restrict__ rotmat, const float* __restrict__ J,
                                                        float* __restrict__ A, float* __restrict__ jt) {
    __shared__ float G[NJ][12];
    const int f = blockIdx.x, lane = threadIdx.x;
    const float* R = rotmat + (size_t)f * NJ * 9;
    const float* Jf = J + (size_t)f * NJ * 3;
    const int r = lane >> 2, c = lane & 3;
    for (int i = 0; i < NJ; ++i) {
        if (lane < 12) {
            const int par = c_parents[i];
            float val;
            if (par < 0) {
                val = c < 3 ? R[i * 9 + r * 3 + c] : Jf[i * 3 + r];
            } else {
                const float* g = G[par] + r * 4;
                if (c < 3) {
                    val = fmaf(g[2], R[i * 9 + 6 + c], fmaf(g[1], R[i * 9 + 3 + c], g[0] * R[i * 9 + c]));
                } else {
                    const float t0 = Jf[i * 3 + 0] - Jf[par * 3 + 0], t1 = Jf[i * 3 + 1] - Jf[par * 3 + 1], t2 = Jf[i * 3 + 2] - Jf[par * 3 + 2];
                    val = fmaf(g[2], t2, fmaf(g[1], t1, g[0] * t0)) + g[3];
                }
            }
            G[i][lane] = val;
        }
        __syncthreads();
    }
    for (int k = lane; k < NJ * 12; k += 64) {
        const int i = k / 12, e = k - i * 12, rr = e >> 2, cc = e & 3;
        float val = G[i][e];
        if (cc == 3) {
            const float* g = G[i] + rr * 4;
            jt[((size_t)f * NJ + i) * 3 + rr] = val;
            val = val - fmaf(g[2], Jf[i * 3 + 2], fmaf(g[1], Jf[i * 3 + 1], g[0] * Jf[i * 3 + 0]));
        }
        A[(size_t)f * NJ * 12 + k] = val;
    }
}

__global__ __launch_bounds__(256) void smpl_skin_kernel(const float* __restrict__ weights, const float* __restrict__ A,
                                                        const float* __restrict__ v_posed, float* __restrict__ verts, int V) {
    __shared__ float sA[NJ * 12];
    const int f = blockIdx.y;
    for (int k = threadIdx.x; k < NJ * 12; k += 256) sA[k] = A[(size_t)f * NJ * 12 + k];
    __syncthreads();
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const float* w = weights + (size_t)v * NJ;
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.f;
    for (int i = 0; i < NJ; ++i) {
        const float wi = w[i];
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = fmaf(wi, sA[i * 12 + e], T[e]);
    }
    const float* p = v_posed + ((size_t)f * V + v) * 3;
    const float x = p[0], y = p[1], z = p[2];
    float* o = verts + ((size_t)f * V + v) * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = fmaf(T[r * 4 + 2], z, fmaf(T[r * 4 + 1], y, T[r * 4 + 0] * x)) + T[r * 4 + 3];
}

// SPIN's rotation_matrix_to_angle_axis (torchgeometry: quaternion branches on the TRANSPOSED matrix, eps 1e-6), in double
__device__ void rotmat_to_aa(const float* R, float* aa) {
    // m(i, j) = rmat_t[i][j] = R[j][i]
#define M_(i, j) ((double)R[(j) * 3 + (i)])
    const double m00 = M_(0, 0), m01 = M_(0, 1), m02 = M_(0, 2), m10 = M_(1, 0), m11 = M_(1, 1), m12 = M_(1, 2), m20 = M_(2, 0),
                 m21 = M_(2, 1), m22 = M_(2, 2);
#undef M_
    double q[4], t;
    if (m22 < 1e-6) {
        if (m00 > m11) {
            t = 1 + m00 - m11 - m22;
            q[0] = m12 - m21; q[1] = t; q[2] = m01 + m10; q[3] = m20 + m02;
        } else {
            t = 1 - m00 + m11 - m22;
            q[0] = m20 - m02; q[1] = m01 + m10; q[2] = t; q[3] = m12 + m21;
        }
    } else {
        if (m00 < -m11) {
            t = 1 - m00 - m11 + m22;
            q[0] = m01 - m10; q[1] = m20 + m02; q[2] = m12 + m21; q[3] = t;
        } else {
            t = 1 + m00 + m11 + m22;
            q[0] = t; q[1] = m12 - m21; q[2] = m20 - m02; q[3] = m01 - m10;
        }
    }
    const double sc = 0.5 / sqrt(t);
    for (int k = 0; k < 4; ++k) q[k] *= sc;
    const double sin_sq = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const double sin_t = sqrt(sin_sq), cos_t = q[0];
    const double two_theta = 2.0 * (cos_t < 0.0 ? atan2(-sin_t, -cos_t) : atan2(sin_t, cos_t));
    const double k = sin_sq > 0.0 ? two_theta / sin_t : 2.0;
    for (int e = 0; e < 3; ++e) {
        const double a = q[1 + e] * k;
        aa[e] = (a != a) ? 0.f : (float)a;
    }
}

__global__ __launch_bounds__(64) void smpl_joints_kernel(const float* __restrict__ jt, const float* __restrict__ verts,
                                                         const float* __restrict__ jx, const int* __restrict__ vertex_ids,
                                                         const int* __restrict__ joint_map, const float* __restrict__ cam,
                                                         const float* __restrict__ rotmat, int V, float* __restrict__ joints3d,
                                                         float* __restrict__ kp2d, float* __restrict__ pose_aa) {
    const int f = blockIdx.x, k = threadIdx.x;
    if (k < NOUT) {
        const int src = joint_map[k];
        const float* p;
        if (src < NJ) p = jt + ((size_t)f * NJ + src) * 3;
        else if (src < NJ + NPICK) p = verts + ((size_t)f * V + vertex_ids[src - NJ]) * 3;
        else p = jx + ((size_t)f * NEXTRA + (src - NJ - NPICK)) * 3;
        const float x = p[0], y = p[1], z = p[2];
        float* o = joints3d + ((size_t)f * NOUT + k) * 3;
        o[0] = x; o[1] = y; o[2] = z;
        const float* c = cam + (size_t)f * 3;
        const float tz = (2.f * 5000.f) / (224.f * c[0] + 1e-9f);
        const float px = x + c[1], py = y + c[2], pz = z + tz;
        kp2d[((size_t)f * NOUT + k) * 2 + 0] = ((px / pz) * 5000.f) / 112.f;
        kp2d[((size_t)f * NOUT + k) * 2 + 1] = ((py / pz) * 5000.f) / 112.f;
    }
    if (k < NJ) rotmat_to_aa(rotmat + ((size_t)f * NJ + k) * 9, pose_aa + ((size_t)f * NJ + k) * 3);
}

__global__ __launch_bounds__(64) void vibe_unpack_kernel(const float* __restrict__ pose6d, const float* __restrict__ shape, int shape_stride,
                                                         const float* __restrict__ cam_in, int cam_stride, float* __restrict__ rotmat,
                                                         float* __restrict__ betas, float* __restrict__ cam) {
    const int f = blockIdx.x, k = threadIdx.x;
    if (k < NJ) {
        const float* a = pose6d + (size_t)f * 144 + k * 6;      // viewed [3][2]: a1 = (a[0], a[2], a[4]), a2 = (a[1], a[3], a[5])
        const float a1x = a[0], a1y = a[2], a1z = a[4], a2x = a[1], a2y = a[3], a2z = a[5];
        const float n1 = fmaxf(sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12f);
        const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
        const float d = b1x * a2x + b1y * a2y + b1z * a2z;
        const float ux = a2x - d * b1x, uy = a2y - d * b1y, uz = a2z - d * b1z;
        const float n2 = fmaxf(sqrtf(ux * ux + uy * uy + uz * uz), 1e-12f);
        const float b2x = ux / n2, b2y = uy / n2, b2z = uz / n2;
        const float b3x = b1y * b2z - b1z * b2y, b3y = b1z * b2x - b1x * b2z, b3z = b1x * b2y - b1y * b2x;
        float* R = rotmat + ((size_t)f * NJ + k) * 9;
        R[0] = b1x; R[1] = b2x; R[2] = b3x;
        R[3] = b1y; R[4] = b2y; R[5] = b3y;
        R[6] = b1z; R[7] = b2z; R[8] = b3z;
    } else if (k < NJ + NB) {
        betas[(size_t)f * NB + (k - NJ)] = shape[(size_t)f * shape_stride + (k - NJ)];
    } else if (k < NJ + NB + 3) {
        cam[(size_t)f * 3 + (k - NJ - NB)] = cam_in[(size_t)f * cam_stride + (k - NJ - NB)];
    }
}

}  // namespace

struct pp_smpl_model {
    int device = 0;
    int V = 0;
    float* blob = nullptr;      // one allocation: the six arrays below, then the two index tables
    const float *v_template = nullptr, *shapedirs = nullptr, *posedirs = nullptr, *j_reg = nullptr, *weights = nullptr, *j_extra = nullptr;
    const int *vertex_ids = nullptr, *joint_map = nullptr;
};

extern "C" int pp_smpl_model_create(pp_ctx* ctx, const float* v_template, const float* shapedirs, const float* posedirs,
                                    const float* j_regressor, const float* weights, const float* j_regressor_extra, int n_verts,
                                    const int32_t* vertex_ids, const int32_t* joint_map, pp_smpl_model** out) {
    PP_REQUIRE(ctx && v_template && shapedirs && posedirs && j_regressor && weights && j_regressor_extra && vertex_ids && joint_map && out,
               "pp_smpl_model_create: NULL argument");
    PP_REQUIRE(n_verts >= 1 && n_verts <= (1 << 20), "pp_smpl_model_create: %d vertices", n_verts);
    for (int k = 0; k < NPICK; ++k)
        PP_REQUIRE(vertex_ids[k] >= 0 && vertex_ids[k] < n_verts, "pp_smpl_model_create: vertex_ids[%d] = %d of %d vertices", k, vertex_ids[k], n_verts);
    for (int k = 0; k < NOUT; ++k)
        PP_REQUIRE(joint_map[k] >= 0 && joint_map[k] < NJ54, "pp_smpl_model_create: joint_map[%d] = %d of %d joints", k, joint_map[k], NJ54);
    PP_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t V = (size_t)n_verts;
    const size_t sizes[6] = {V * 3, V * 3 * NB, (size_t)NPF * V * 3, (size_t)NJ * V, V * NJ, (size_t)NEXTRA * V};
    const float* src[6] = {v_template, shapedirs, posedirs, j_regressor, weights, j_regressor_extra};
    size_t total = 0, off[6];
    for (int k = 0; k < 6; ++k) {
        off[k] = total;
        total += (sizes[k] + 3) & ~size_t(3);
    }
    pp_smpl_model* m = new pp_smpl_model();
    m->device = ctx->device;
    m->V = n_verts;
    if (hipMalloc(&m->blob, (total + NPICK + NOUT + 2) * sizeof(float)) != hipSuccess) {
        delete m;
        pp_set_error("pp_smpl_model_create: out of device memory");
        return PP_ERR_HIP;
    }
    hipError_t e = hipSuccess;
    for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipMemcpy(m->blob + off[k], src[k], sizes[k] * sizeof(float), hipMemcpyHostToDevice);
    int* ids = reinterpret_cast<int*>(m->blob + total);
    if (e == hipSuccess) e = hipMemcpy(ids, vertex_ids, NPICK * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ids + NPICK, joint_map, NOUT * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(m->blob);
        delete m;
        pp_set_error("pp_smpl_model_create: upload failed: %s", hipGetErrorString(e));
        return PP_ERR_HIP;
    }
    m->v_template = m->blob + off[0]; m->shapedirs = m->blob + off[1]; m->posedirs = m->blob + off[2];
    m->j_reg = m->blob + off[3]; m->weights = m->blob + off[4]; m->j_extra = m->blob + off[5];
    m->vertex_ids = ids; m->joint_map = ids + NPICK;
    *out = m;
    return PP_OK;
}

extern "C" void pp_smpl_model_destroy(pp_smpl_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipFree(m->blob);
    delete m;
}

namespace {
int smpl_enqueue(pp_ctx* ctx, const pp_smpl_model* m, const float* betas, const float* rotmat, const float* cam, int F, float* verts,
                 float* joints3d, float* kp2d, float* pose_aa, bool host) {
    hipStream_t s = ctx->stream;
    const size_t V = (size_t)m->V, V3 = V * 3, nF = (size_t)F;
    const size_t e_b = nF * NB, e_r = nF * NJ * 9, e_c = nF * 3, e_v = nF * V3, e_j = nF * NOUT * 3, e_k = nF * NOUT * 2, e_a = nF * NJ * 3;
    auto al = [](size_t e) { return ScratchCursor::align(e * sizeof(float)); };
    // work: v_shaped, v_posed, verts (when not returned to a device caller), J, A, jt, jx
    size_t need = 3 * al(e_v) + al(nF * NJ * 3) + al(nF * NJ * 12) + al(nF * NJ * 3) + al(nF * NEXTRA * 3);
    if (host) need += al(e_b) + al(e_r) + al(e_c) + al(e_j) + al(e_k) + al(e_a);
    int rc = ctx->ensure_scratch(need);
    if (rc != PP_OK) return rc;
    ScratchCursor cur(ctx);
    float* v_shaped = cur.take<float>(e_v);
    float* v_posed = cur.take<float>(e_v);
    float* w_verts = cur.take<float>(e_v);
    float* J = cur.take<float>(nF * NJ * 3);
    float* A = cur.take<float>(nF * NJ * 12);
    float* jt = cur.take<float>(nF * NJ * 3);
    float* jx = cur.take<float>(nF * NEXTRA * 3);
    const float *d_b = betas, *d_r = rotmat, *d_c = cam;
    float *d_v = (!host && verts) ? verts : w_verts, *d_j = joints3d, *d_k = kp2d, *d_a = pose_aa;
    if (host) {
        float* sb = cur.take<float>(e_b);
        float* sr = cur.take<float>(e_r);
        float* sc = cur.take<float>(e_c);
        d_j = cur.take<float>(e_j);
        d_k = cur.take<float>(e_k);
        d_a = cur.take<float>(e_a);
        PP_HIP_CHECK(hipMemcpyAsync(sb, betas, e_b * 4, hipMemcpyHostToDevice, s));
        PP_HIP_CHECK(hipMemcpyAsync(sr, rotmat, e_r * 4, hipMemcpyHostToDevice, s));
        PP_HIP_CHECK(hipMemcpyAsync(sc, cam, e_c * 4, hipMemcpyHostToDevice, s));
        d_b = sb; d_r = sr; d_c = sc;
    }
    const dim3 gv((unsigned)((V3 + 255) / 256), (unsigned)F), gs((unsigned)((V + 255) / 256), (unsigned)F);
    hipLaunchKernelGGL(smpl_shape_kernel, gv, dim3(256), 0, s, m->v_template, m->shapedirs, d_b, v_shaped, (int)V3);
    hipLaunchKernelGGL(smpl_regress_kernel, dim3(NJ, (unsigned)F), dim3(256), 0, s, m->j_reg, v_shaped, J, (int)V, NJ);
    hipLaunchKernelGGL(smpl_pose_kernel, gv, dim3(256), 0, s, m->posedirs, d_r, v_shaped, v_posed, (int)V3);
    hipLaunchKernelGGL(smpl_chain_kernel, dim3((unsigned)F), dim3(64), 0, s, d_r, J, A, jt);
    hipLaunchKernelGGL(smpl_skin_kernel, gs, dim3(256), 0, s, m->weights, A, v_posed, d_v, (int)V);
    hipLaunchKernelGGL(smpl_regress_kernel, dim3(NEXTRA, (unsigned)F), dim3(256), 0, s, m->j_extra, d_v, jx, (int)V, NEXTRA);
    hipLaunchKernelGGL(smpl_joints_kernel, dim3((unsigned)F), dim3(64), 0, s, jt, d_v, jx, m->vertex_ids, m->joint_map, d_c, d_r, (int)V, d_j,
                       d_k, d_a);
    PP_HIP_CHECK(hipGetLastError());
    if (host) {
        if (verts) PP_HIP_CHECK(hipMemcpyAsync(verts, d_v, e_v * 4, hipMemcpyDeviceToHost, s));
        PP_HIP_CHECK(hipMemcpyAsync(joints3d, d_j, e_j * 4, hipMemcpyDeviceToHost, s));
        PP_HIP_CHECK(hipMemcpyAsync(kp2d, d_k, e_k * 4, hipMemcpyDeviceToHost, s));
        PP_HIP_CHECK(hipMemcpyAsync(pose_aa, d_a, e_a * 4, hipMemcpyDeviceToHost, s));
    }
    return PP_OK;
}
}  // namespace

extern "C" int pp_smpl_forward(pp_ctx* ctx, pp_smpl_model* model, const float* betas, const float* rotmat, const float* cam, int F,
                               float* verts, float* joints3d, float* kp2d, float* pose_aa, int mem) {
    PP_REQUIRE(ctx && model && betas && rotmat && cam && joints3d && kp2d && pose_aa, "pp_smpl_forward: NULL argument");
    PP_REQUIRE(mem == PP_MEM_HOST || mem == PP_MEM_DEVICE, "pp_smpl_forward: mem %d is neither PP_MEM_HOST nor PP_MEM_DEVICE", mem);
    PP_REQUIRE(F >= 0 && F <= 65535, "pp_smpl_forward: %d frames in one call (at most 65535)", F);
    PP_REQUIRE(model->device == ctx->device, "pp_smpl_forward: the model lives on device %d, the context on %d", model->device, ctx->device);
    if (F == 0) return PP_OK;
    PP_HIP_CHECK(hipSetDevice(ctx->device));
    PpRange range("pp_smpl_forward");
    const bool host = mem == PP_MEM_HOST;
    int rc = smpl_enqueue(ctx, model, betas, rotmat, cam, F, verts, joints3d, kp2d, pose_aa, host);
    if (host) {
        // queued copies read and write the caller's arrays: complete on return, also after an error
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (rc != PP_OK) return rc;
        PP_HIP_CHECK(e);
    }
    return rc;
}

extern "C" int pp_vibe_head_unpack(pp_ctx* ctx, const float* pose6d, const float* shape, int shape_stride, const float* cam_in,
                                   int cam_stride, int F, float* rotmat, float* betas, float* cam) {
    PP_REQUIRE(ctx && pose6d && shape && cam_in && rotmat && betas && cam, "pp_vibe_head_unpack: NULL argument");
    PP_REQUIRE(shape_stride >= NB && cam_stride >= 3 && F >= 0, "pp_vibe_head_unpack: strides %d / %d, %d frames", shape_stride, cam_stride, F);
    if (F == 0) return PP_OK;
    PP_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(vibe_unpack_kernel, dim3((unsigned)F), dim3(64), 0, ctx->stream, pose6d, shape, shape_stride, cam_in, cam_stride, rotmat,
                       betas, cam);
    PP_HIP_CHECK(hipGetLastError());
    return PP_OK;
}
