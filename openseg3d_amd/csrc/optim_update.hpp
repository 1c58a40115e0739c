// The optimizer step's arithmetic, once: the kernel of optim.hip and its plain-C++ host twin both call these, and the
// library is built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt, so the two agree bit for bit.
// The order of the fp32 operations is that of torch's single-tensor algorithms (torch/optim/sgd.py _single_tensor_sgd,
// torch/optim/adamw.py -> adam.py _single_tensor_adam, the non-capturable branch).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/seg3d_hip.h"

// SGD, dampening 0, no Nesterov.  h->v: [0] lr, [1] weight decay, [2] momentum.  m == nullptr: no momentum, no state.
// first: the tensor's first step, the buffer starts as the (decayed) gradient.
__host__ __device__ inline void sgd_update(float* p, float g, float* m, bool first, const seg3d_optim_hyper* h) {
    const float lr = h->v[0], wd = h->v[1], mu = h->v[2];
    if (wd != 0.f) g = g + wd * *p;
    if (m) {
        g = first ? g : mu * *m + g;
        *m = g;
    }
    *p = *p - lr * g;
}

// AdamW, decoupled decay, no amsgrad.  h->v: [0] 1 - lr * wd, [1] 1 - beta1, [2] beta2, [3] 1 - beta2, [4] lr / bc1,
// [5] sqrt(bc2), [6] eps -- each computed in double on the host from the step count and rounded to float once.
// m + (g - m) * (1 - beta1) is torch's lerp_ for a weight below 0.5, i.e. beta1 > 0.5 (every config, and OneCycleLR's 0.85
// to 0.95); at beta1 <= 0.5 torch's lerp switches to g - (g - m) * beta1 and the order of operations is no longer torch's.
__host__ __device__ inline void adamw_update(float* p, float g, float* m, float* v, const seg3d_optim_hyper* h) {
    const float pd = *p * h->v[0];
    const float mn = *m + (g - *m) * h->v[1];
    const float vn = *v * h->v[2] + h->v[3] * g * g;
    *m = mn;
    *v = vn;
    *p = pd - h->v[4] * mn / (sqrtf(vn) / h->v[5] + h->v[6]);
}
