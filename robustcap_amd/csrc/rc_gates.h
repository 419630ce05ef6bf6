// Gate non-linearities of the LSTM epilogues (rc_gemm.hip, rc_live.hip): one definition, so that every path computes the same bits.
#pragma once
#ifndef RC_FAST_GATES
#define RC_FAST_GATES 1       // on v_exp_f32 / v_rcp_f32 (0: libm expf / tanhf, A/B builds): measured +3.6 % frame rate with parity
#endif                        // margins unchanged (profiles/r02_parity_margins.json)
#if RC_FAST_GATES
__device__ __forceinline__ float rc_gate_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896f * x)); }
// tanh(x) = sign(x) (1 - t) / (1 + t), t = exp(-2 |x|) in (0, 1]: no cancellation near 0 (1 - 2 / (1 + e^2x) loses every
// significant bit of a small x there)
__device__ __forceinline__ float rc_gate_tanh(float x) {
    const float t = __builtin_amdgcn_exp2f(-2.88539008177793f * __builtin_fabsf(x));
    return __builtin_copysignf((1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t), x);
}
#else
__device__ __forceinline__ float rc_gate_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float rc_gate_tanh(float x) { return tanhf(x); }
#endif

// One LSTM cell update from the four gate pre-activations (torch order i, f, g, o; articulate/utils/torch/rnn.py:129-133 -> aten::lstm):
// c' = sigma(f) c + sigma(i) tanh(g), h' = sigma(o) tanh(c'). ONE definition with the contraction written out (fma(f, c, i * g)), so
// that every tile shape of rc_gemm.hip and the shared-weight kernel of rc_gemm_lds.hip produce the same bits.
__device__ __forceinline__ void rc_lstm_cell(float gi, float gf, float gg, float go, float c_prev, float& c_new, float& h_new) {
    const float ig = rc_gate_sigmoid(gi), fg = rc_gate_sigmoid(gf);
    const float cg = rc_gate_tanh(gg), og = rc_gate_sigmoid(go);
    c_new = __builtin_fmaf(fg, c_prev, ig * cg);
    h_new = og * rc_gate_tanh(c_new);
}

// The same update, also returning the four gate activations (the tape of rc_subnet_forward_tape): the operations of rc_lstm_cell in
// its order, so that c' and h' keep their bits.
__device__ __forceinline__ void rc_lstm_cell_acts(float gi, float gf, float gg, float go, float c_prev, float& c_new, float& h_new,
                                                  float& ig, float& fg, float& cg, float& og) {
    ig = rc_gate_sigmoid(gi); fg = rc_gate_sigmoid(gf);
    cg = rc_gate_tanh(gg); og = rc_gate_sigmoid(go);
    c_new = __builtin_fmaf(fg, c_prev, ig * cg);
    h_new = og * rc_gate_tanh(c_new);
}

// One cell of back-propagation through time (eval-mode aten::lstm; the loop of articulate/utils/torch/train.py:117-122 reaches it through
// loss.backward()). In: the recorded activations i, f, g, o, c(t) and c(t - 1), dh = the gradient of h(t) from the layer above plus
// the recurrent one, dc_next = the gradient of c(t) carried from step t + 1. Out: the gradients of the four gate PRE-activations
// (sigma' = s (1 - s), tanh' = 1 - g^2) and dc_prev, the gradient carried to step t - 1. tanh(c) is formed as the forward formed it.
__device__ __forceinline__ void rc_lstm_cell_backward(float ig, float fg, float cg, float og, float c, float c_prev, float dh, float dc_next,
                                                      float& dgi, float& dgf, float& dgg, float& dgo, float& dc_prev) {
    const float tc = rc_gate_tanh(c);
    const float d_o = dh * tc;
    const float dc = dc_next + dh * og * (1.0f - tc * tc);
    const float d_i = dc * cg, d_g = dc * ig, d_f = dc * c_prev;
    dc_prev = dc * fg;
    dgi = d_i * ig * (1.0f - ig);
    dgf = d_f * fg * (1.0f - fg);
    dgg = d_g * (1.0f - cg * cg);
    dgo = d_o * og * (1.0f - og);
}
