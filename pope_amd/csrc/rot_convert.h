// convert2matrix of the fork's pose heads (pose/model.py, pose/model_cnn.py; pose/utils.py:qua2mat, o6d2mat): the rotation
// head's output -> a row-major 3 x 3 matrix, fp32.  One definition for the key-point regressor (pose_regressor.hip) and the image
// pose head (convnext.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/pope_hip.h"  // POPE_ROT_*

__device__ __forceinline__ void pope_rot_normalize(const float* v, int n, float* o) {   // pose/utils.py:normalize_vector (norm clamped at 1e-8)
    float ss = 0.f;
    for (int i = 0; i < n; ++i) ss += v[i] * v[i];
    const float mag = fmaxf(sqrtf(ss), 1e-8f);
    for (int i = 0; i < n; ++i) o[i] = v[i] / mag;
}

// r: 9 (POPE_ROT_MATRIX), 4 (POPE_ROT_QUAT) or 6 (POPE_ROT_6D) values; r_out [9]
__device__ __forceinline__ void pope_rot_to_matrix(int mode, const float* r, float* r_out) {
    if (mode == POPE_ROT_MATRIX) {
        for (int i = 0; i < 9; ++i) r_out[i] = r[i];
    } else if (mode == POPE_ROT_QUAT) {     // pose/utils.py:qua2mat, (w, x, y, z)
        float q[4];
        pope_rot_normalize(r, 4, q);
        const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
        const float xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, xw = qx * qw, yw = qy * qw, zw = qz * qw;
        r_out[0] = 1 - 2 * yy - 2 * zz; r_out[1] = 2 * xy - 2 * zw;     r_out[2] = 2 * xz + 2 * yw;
        r_out[3] = 2 * xy + 2 * zw;     r_out[4] = 1 - 2 * xx - 2 * zz; r_out[5] = 2 * yz - 2 * xw;
        r_out[6] = 2 * xz - 2 * yw;     r_out[7] = 2 * yz + 2 * xw;     r_out[8] = 1 - 2 * xx - 2 * yy;
    } else {                                   // pose/utils.py:o6d2mat: x, y, z are the COLUMNS
        float x[3], y[3], z[3], zr[3];
        pope_rot_normalize(r, 3, x);
        const float* yr = r + 3;
        zr[0] = x[1] * yr[2] - x[2] * yr[1]; zr[1] = x[2] * yr[0] - x[0] * yr[2]; zr[2] = x[0] * yr[1] - x[1] * yr[0];
        pope_rot_normalize(zr, 3, z);
        y[0] = z[1] * x[2] - z[2] * x[1]; y[1] = z[2] * x[0] - z[0] * x[2]; y[2] = z[0] * x[1] - z[1] * x[0];
        for (int i = 0; i < 3; ++i) { r_out[3 * i] = x[i]; r_out[3 * i + 1] = y[i]; r_out[3 * i + 2] = z[i]; }
    }
}
