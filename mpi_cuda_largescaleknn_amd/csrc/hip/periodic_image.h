// The image helpers of the periodic walks (periodic.hip, knn_periodic.hip): a group's axes
// against the root box, the images it can take, the slackened gaps of the conservative cull,
// the whole-box acceptance and the minimum image of the difference for the bucket scan.
// periodic.hip states the contract and proves each step.
#pragma once
#include "ball_walk.h"

namespace lsk {
namespace periodic {

constexpr float kSlack = 0x1p-21f;  // periodic.hip: "The cull is conservative"

// One axis of the period as a group sees it (wave-uniform).
struct Axis {
  float L, h, e;  // period, half period, slack of a shifted gap
  bool neg, pos;  // some pair (group query, root point) may take s = -1 / s = +1
};

__device__ __forceinline__ Axis make_axis(float L, float qlo, float qhi, float plo, float phi) {
  Axis a;
  a.L = L;
  a.h = 0.5f * L;
  a.neg = qhi - plo > a.h;
  a.pos = qlo - phi < -a.h;
  a.e = kSlack * (fmaxf(fabsf(qlo), fabsf(qhi)) + fmaxf(fabsf(plo), fabsf(phi)) + L);
  return a;
}

// The shift of one axis in the current image: s, the offset o = s L of the query and the
// slack e of the axis' gap (both 0 where s = 0, so that image 0 is the open-box arithmetic).
struct Shift {
  int s;
  float o, e;
};

__device__ __forceinline__ bool shift_of(const Axis &a, int s, Shift &S) {
  S.s = s;
  S.o = 0.f;
  S.e = 0.f;
  if (s == 0) return true;
  if (s < 0 ? !a.neg : !a.pos) return false;
  S.o = s < 0 ? -a.L : a.L;
  S.e = a.e;
  return true;
}

struct Image {
  Shift x, y, z;
};

// Image im in [0, 27) of the group, or false when no pair can take it.
__device__ __forceinline__ bool image_of(const Axis &X, const Axis &Y, const Axis &Z, int im, Image &I) {
  const int sx = im % 3 - 1, sy = (im / 3) % 3 - 1, sz = im / 9 - 1;
  const bool ok_x = shift_of(X, sx, I.x), ok_y = shift_of(Y, sy, I.y), ok_z = shift_of(Z, sz, I.z);
  return ok_x && ok_y && ok_z;
}

// The minimum image of one difference and the branch it took.
__device__ __forceinline__ float wrap1(float d, float L, float h, int &w) {
  w = 0;
  if (d > h) {
    d = d - L;
    w = -1;
  } else if (d < -h) {
    d = d + L;
    w = 1;
  }
  return d;
}

// Gap of one axis between the query range [qlo, qhi] moved by the image and [lo, hi].
__device__ __forceinline__ float gap1(float qlo, float qhi, float lo, float hi, const Shift &S) {
  const float g = fmaxf(fmaxf(lo - (qhi + S.o), (qlo + S.o) - hi), 0.f);
  return fmaxf(g - S.e, 0.f);
}

__device__ __forceinline__ float image_box_dist2(const lsk::box3f &gb, const float4 &lo4, const float4 &hi4,
                                                 const Image &I) {
  return lsk::dist2(gap1(gb.lo.x, gb.hi.x, lo4.x, hi4.x, I.x), gap1(gb.lo.y, gb.hi.y, lo4.y, hi4.y, I.y),
                    gap1(gb.lo.z, gb.hi.z, lo4.z, hi4.z, I.z));
}

__device__ __forceinline__ float image_point_dist2(const lsk::GroupQuery &Q, const float4 &lo4, const float4 &hi4,
                                                   const Image &I) {
  return lsk::dist2(gap1(Q.x, Q.x, lo4.x, hi4.x, I.x), gap1(Q.y, Q.y, lo4.y, hi4.y, I.y),
                    gap1(Q.z, Q.z, lo4.z, hi4.z, I.z));
}

// One axis of the whole-box acceptance: both corners take branch s; f = the larger |wrapped
// corner difference|.
__device__ __forceinline__ bool far1(float q, float lo, float hi, const Axis &a, int s, float &f) {
  int wl, wh;
  const float dl = wrap1(q - lo, a.L, a.h, wl), dh = wrap1(q - hi, a.L, a.h, wh);
  f = fmaxf(fabsf(dl), fabsf(dh));
  return wl == s && wh == s;
}

// All of the node belongs to image I for the lane; far = the canonical dist2 of the per-axis
// larger |wrapped corner difference|, an upper bound of every point's pd2 when it does.
__device__ __forceinline__ bool box_far(const lsk::GroupQuery &Q, const float4 &lo4, const float4 &hi4,
                                        const Axis &X, const Axis &Y, const Axis &Z, const Image &I, float &far) {
  float fx, fy, fz;
  const bool in_x = far1(Q.x, lo4.x, hi4.x, X, I.x.s, fx), in_y = far1(Q.y, lo4.y, hi4.y, Y, I.y.s, fy),
             in_z = far1(Q.z, lo4.z, hi4.z, Z, I.z.s, fz);
  far = lsk::dist2(fx, fy, fz);
  return in_x && in_y && in_z;
}

// All of the node belongs to image I for the lane, and its farthest point is below cut2.
__device__ __forceinline__ bool box_inside(const lsk::GroupQuery &Q, const float4 &lo4, const float4 &hi4,
                                           const Axis &X, const Axis &Y, const Axis &Z, const Image &I, float cut2) {
  float far;
  return box_far(Q, lo4, hi4, X, Y, Z, I, far) && far < cut2;
}

// The group's three axes against the root box.
struct Frame {
  Axis X, Y, Z;
  float4 rlo, rhi;  // the root's box
};

__device__ __forceinline__ Frame make_frame(const lsk_tree_view &T, const float *L, const lsk::box3f &gb) {
  const float4 *nodes = (const float4 *)T.nodes;
  const float4 lo = nodes[2], hi = nodes[3];
  Frame F;
  F.rlo = make_float4(lsk::uniform_f(lo.x), lsk::uniform_f(lo.y), lsk::uniform_f(lo.z), 0.f);
  F.rhi = make_float4(lsk::uniform_f(hi.x), lsk::uniform_f(hi.y), lsk::uniform_f(hi.z), 0.f);
  F.X = make_axis(L[0], gb.lo.x, gb.hi.x, F.rlo.x, F.rhi.x);
  F.Y = make_axis(L[1], gb.lo.y, gb.hi.y, F.rlo.y, F.rhi.y);
  F.Z = make_axis(L[2], gb.lo.z, gb.hi.z, F.rlo.z, F.rhi.z);
  return F;
}

// The difference of scan_bucket (ball_walk.h) under the period: pd2 of the minimum image, and
// `mine` = the pair's wrap vector is the image's.
struct ImageDiff {
  const Frame &F;
  const Image &I;
  __device__ __forceinline__ float operator()(const lsk::GroupQuery &Q, float x, float y, float z,
                                              bool &mine) const {
    int wx, wy, wz;
    const float dx = wrap1(Q.x - x, F.X.L, F.X.h, wx), dy = wrap1(Q.y - y, F.Y.L, F.Y.h, wy),
                dz = wrap1(Q.z - z, F.Z.L, F.Z.h, wz);
    mine = wx == I.x.s && wy == I.y.s && wz == I.z.s;
    return lsk::dist2(dx, dy, dz);
  }
};

}  // namespace periodic
}  // namespace lsk
