// Host-side helpers the extractors share: the cursor over the packed weight buffer, the record of a GEMM layer in it, filling a GemmP
// from that record, the name table of a state dict and the float32 BatchNorm fold.  Host code only; nothing here launches a kernel.
#pragma once
#include <math.h>

#include <string>
#include <vector>

#include "gemm.h"

// cursor over the packed buffer: every entry starts on a 64-float slot
struct PackCursor {
    size_t off = 0;
    size_t get(size_t n) {
        const size_t o = off;
        off += align_up(n, 64);
        return o;
    }
};

// A GEMM layer [nrows][K] in the packed buffer: f32 weights, bias [nrows], the two fragment-major f16 planes of the split arithmetic
// (rows padded to 32) and their scale, in this order.
struct GemmLayerOff {
    size_t w = 0, b = 0, wh = 0, wl = 0, ws = 0;
    void place(PackCursor& c, int nrows, int K) {
        const size_t np = align_up((size_t)nrows, 32);
        w = c.get((size_t)nrows * K);
        b = c.get(nrows);
        wh = c.get(np * K / 2);
        wl = c.get(np * K / 2);
        ws = c.get(1);
    }
    // the f16 planes and the scale of the f32 weights already at packed + w
    void split_planes(float* packed, int nrows, int K) const {
        unsigned short* hi = reinterpret_cast<unsigned short*>(packed + wh);
        unsigned short* lo = reinterpret_cast<unsigned short*>(packed + wl);
        packed[ws] = split_weights_frag_host(packed + w, nrows, K, hi, lo);
    }
};

// W [N][K] (K-contiguous), bias and, for the split arithmetic, the pre-split planes of layer `o` of the packed buffer P
static inline void gemm_set_weights(GemmP& g, const float* P, const GemmLayerOff& o, int N, int K, bool split) {
    g.W = P + o.w;
    g.ldw = K;
    g.bias = P + o.b;
    g.N = N;
    g.K = K;
    if (split) {
        g.Wh = reinterpret_cast<const unsigned short*>(P + o.wh);
        g.Wl = reinterpret_cast<const unsigned short*>(P + o.wl);
        g.wscale = P + o.ws;
    }
}
// implicit im2col: A is the NHWC map [B, hin, win, cin], row m of the GEMM is output pixel m
static inline void gemm_set_conv(GemmP& g, int k, int stride, int pad, int hin, int win, int hout, int wout, int cin) {
    g.conv_k = k;
    g.conv_stride = stride;
    g.conv_pad = pad;
    g.conv_hin = hin;
    g.conv_win = win;
    g.conv_hout = hout;
    g.conv_wout = wout;
    g.conv_cin = cin;
}

// the tensors of a state dict in the order the packer takes them: name and element count
struct TensorTable {
    struct Entry {
        std::string name;
        size_t n;
    };
    std::vector<Entry> t;
    void add(const std::string& name, size_t n) { t.push_back({name, n}); }
    int size() const { return (int)t.size(); }
    const char* name(int i) const { return (i < 0 || i >= size()) ? nullptr : t[i].name.c_str(); }
    int find(const std::string& name) const {
        for (size_t i = 0; i < t.size(); ++i)
            if (t[i].name == name) return (int)i;
        return -1;
    }
};

// BatchNorm2d (eval, eps 1e-5) folded into the convolution before it, in float32: w' = w * scale, b' = shift with
// scale = g / sqrt(var + eps), shift = beta - mean * scale.  bn = the four tensors weight, bias, running_mean, running_var.
static inline void bn_fold_f32(const float* const* bn, int cout, std::vector<float>& scale, std::vector<float>& shift) {
    scale.assign(cout, 1.0f);
    shift.assign(cout, 0.0f);
    for (int c = 0; c < cout; ++c) {
        const float s = bn[0][c] / sqrtf(bn[3][c] + 1e-5f);
        scale[c] = s;
        shift[c] = bn[1][c] - bn[2][c] * s;
    }
}
