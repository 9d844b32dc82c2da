// tb_render.hpp -- rgb_array frames of env states: one primary ray per pixel against the five analytic primitives of the scene,
// the nearest hit kept. Additive: it reads state words and writes images, no step / policy / learner kernel knows of it.
//
// THE RULE (tests/render_reference.py restates it in numpy from this text, not from the code below)
//
// Camera. f = unit(target - eye), r = unit(f x up), u = r x f, th = tan(fov_y / 2): computed once on the host in float64 and
// handed over as float32 f, th (W / H) r and th u. Pixel (i, j) -- column i to the right, row j downwards, origin top-left --
// looks through its centre: sx = (2 i + 1 - W) / W, sy = (H - 2 j - 1) / H (the integer numerators are exact), direction
// d = unit(f + sx th (W / H) r + sy th u). With follow = 1 the eye of image k is fl(COM_k + eye) in float32, COM_k the racket COM of
// the env the image shows, and f, r, u come from target - eye as given: the view direction does not depend on the env.
//
// Primitives, every one convex, visited in the order of their ids; a later one replaces an earlier one only where strictly nearer:
//   1 ground  the box |x| <= ground_half[0], |y| <= ground_half[1], |z| <= ground_half[2]          (sphere_vs_box's, tb_device.hpp)
//   2 net     the box of net_half, only with TB_F_NET
//   3 goal    SwingRacket-v0 only: the cylinder (x - gx)^2 + (y - gy)^2 <= goal_radius^2, |z| <= goal_half_len (sphere_vs_goal's)
//   4 ball    the sphere of ball_radius around the ball position
//   5 racket  in the body frame (ray origin and direction rotated by the conjugate quaternion about the COM): the slab
//             |x| <= racket_half_thick s cut by the n_hull half-planes n_i . ((y, z) - s a_i) <= 0, n_i = (e_i.z, -e_i.y) the outward
//             normal of edge i of the CCW outline. s is TbParams.racket_scale on SwingRacket-v0 and the env's own TB_W_TN_SCALE word on
//             Tennisbot-v0. hull_margin -- the 1 mm collision margin around the hull -- is NOT drawn: the picture shows the mesh.
// A ray meets a convex solid for t in [t0, t1]: t0 the largest entry parameter of its constraints, t1 the smallest exit. A slab
// |c| <= h with direction component 0 constrains nothing when |origin component| <= h and rejects the ray otherwise; a half-plane
// with n . d = 0 likewise by the sign of n . (o - s a). Sphere and cylinder use the closest-approach form: tm = -(oc . d) / (d . d),
// p = oc + tm d, h^2 = (R^2 - p . p) / (d . d), t = tm -+ h (the cylinder in (x, y) only, then its z slab; a ray along the axis is
// inside iff oc . oc <= R^2). The solid is hit iff t0 <= t1, at t = t0 when t0 >= 0, else -- the eye is inside -- at t1 when t1 >= 0.
// The normal n is the outward normal of the constraint that gave t, negated for an exit hit: it always faces the eye.
// depth = t (d is a unit vector), +inf where nothing is hit (sky, id 0).
//
// Shading. colour = base[id] * (0.35 + 0.65 max(0, n . l)), l the unit light direction, n . l capped at 1; a ground pixel whose hit
// point lies within 2 ball_radius of the ball's (x, y) while ball.z > ground_half[2] is halved (the drop shadow: without it the
// ball's height cannot be read); sky is base[0]. Each channel is rounded to nearest: (int)(c + 0.5).
//   base: sky (135, 190, 235), ground (60, 140, 80), net (235, 235, 235), goal (220, 60, 50), ball (230, 240, 40), racket (40, 60, 200)
//
// Exceptional values. Every acceptance test is written so that a NaN fails it. A primitive whose state is not finite (ball position;
// goal; racket COM, quaternion or scale, a scale <= 0 too) is not hit; an eye that is not finite (follow = 1 on such a COM) gives
// an all-sky image. No colour is NaN, no id is outside 0..5, no depth is negative or NaN.
//
// Layout: one lane is one pixel, one wave an 8 x 8 tile of ONE image, so the env's state row, the camera and the hull table (kernel
// arguments, 1 KB) are wave-uniform and only the ray is per lane. A wave vote on the racket's bounding sphere skips the edge loop
// for tiles that cannot see it. Stores: where W % 4 == 0 and the base is aligned, four neighbouring lanes pack their 12 colour bytes
// into three dwords and their four ids into one; otherwise bytes. Lanes beyond the image are masked, never clamped.
#pragma once

namespace tb {

struct RenderCam {
  float eye[3], fwd[3], right[3], up[3], light[3];  // right = th (W / H) r, up = th u
  int follow;
};
struct RenderScene {
  float ground_half[3], net_half[3];
  float goal_radius, goal_half_len, ball_radius, half_thick, bound_radius, racket_scale;
  int n_hull;
  uint32_t flags;
};
struct RenderHull { float4 e[TB_MAX_HULL]; };  // a.y a.z e.y e.z at scale 1

// the ray is inside a convex solid for t in [t0, t1]; n0 / n1: outward normals of the constraints that gave them (not normalised)
struct Span { float t0, t1; vec3 n0, n1; bool ok; };
TB_DEV Span span_all() { Span s; s.t0 = -INFINITY; s.t1 = INFINITY; s.n0 = mk(0, 0, 0); s.n1 = mk(0, 0, 0); s.ok = true; return s; }
TB_DEV bool finite1(float x) { return fabsf(x) < INFINITY; }
TB_DEV bool finite3(vec3 v) { return finite1(v.x) && finite1(v.y) && finite1(v.z); }

// one constraint crossed at t with outward normal n; den = n . d < 0: the ray enters through it
TB_DEV void clip(Span& s, float t, bool enters, vec3 n) {
  if (enters) { if (t > s.t0) { s.t0 = t; s.n0 = n; } }
  else if (t < s.t1) { s.t1 = t; s.n1 = n; }
}
TB_DEV void clip_slab(Span& s, float o, float d, float h, vec3 axis) {  // |o + t d| <= h
  if (d != 0.0f) {
    const float inv = 1.0f / d;
    const bool pos = d > 0.0f;
    const vec3 from = pos ? -1.0f * axis : axis;  // outward normal of the face on the side the ray comes from
    clip(s, ((pos ? -h : h) - o) * inv, true, from);
    clip(s, ((pos ? h : -h) - o) * inv, false, -1.0f * from);
  } else if (!(fabsf(o) <= h)) s.ok = false;
}
TB_DEV Span ray_box(vec3 o, vec3 d, const float* half) {
  Span s = span_all();
  clip_slab(s, o.x, d.x, half[0], mk(1, 0, 0));
  clip_slab(s, o.y, d.y, half[1], mk(0, 1, 0));
  clip_slab(s, o.z, d.z, half[2], mk(0, 0, 1));
  return s;
}
// disc or ball of radius R around the origin in the first `dims` components of oc: closest-approach form
TB_DEV void clip_round(Span& s, vec3 oc, vec3 d, float R, bool flat) {
  if (flat) { oc.z = 0.0f; d.z = 0.0f; }
  const float a = dot(d, d);
  if (a != 0.0f) {
    const float tm = -dot(oc, d) / a;
    const vec3 p = fma3(tm, d, oc);
    const float h2 = (R * R - dot(p, p)) / a;
    if (h2 >= 0.0f) {
      const float h = sqrtf(h2);
      clip(s, tm - h, true, fma3(-h, d, p));
      clip(s, tm + h, false, fma3(h, d, p));
    } else s.ok = false;
  } else if (!(dot(oc, oc) <= R * R)) s.ok = false;
}

struct Nearest { float t; vec3 n; int id; };
TB_DEV void take(Nearest& best, const Span& s, int id) {
  if (!(s.ok && s.t0 <= s.t1)) return;
  const bool entry = s.t0 >= 0.0f;
  const float t = entry ? s.t0 : s.t1;
  if (t >= 0.0f && t < best.t) { best.t = t; best.n = entry ? s.n0 : -1.0f * s.n1; best.id = id; }
}

template <int KIND>
__global__ __launch_bounds__(64) void tb_render_kernel(RenderCam cam, RenderScene sc, RenderHull hull, const uint32_t* __restrict__ words, int n_envs,
                                                       const int32_t* __restrict__ env_idx, int W, int H, int tiles_x, int tiles,
                                                       uint8_t* __restrict__ rgb, uint8_t* __restrict__ ids, float* __restrict__ depth) {
  const unsigned img = blockIdx.x / (unsigned)tiles, tile = blockIdx.x % (unsigned)tiles;
  const int lane = threadIdx.x, lx = lane & 7, ly = lane >> 3;
  const int px = (int)(tile % (unsigned)tiles_x) * 8 + lx, py = (int)(tile / (unsigned)tiles_x) * 8 + ly;

  // ---- the env's state row: wave-uniform addresses
  int e = env_idx ? env_idx[img] : (int)img;
  e = e < 0 ? 0 : (e > n_envs - 1 ? n_envs - 1 : e);
  auto word = [&](int row) { return __uint_as_float(words[(size_t)row * (size_t)n_envs + (size_t)e]); };
  const vec3 com = mk(word(TB_W_RP), word(TB_W_RP + 1), word(TB_W_RP + 2));
  quat q; q.x = word(TB_W_RQ); q.y = word(TB_W_RQ + 1); q.z = word(TB_W_RQ + 2); q.w = word(TB_W_RQ + 3);
  const vec3 ball = mk(word(TB_W_BP), word(TB_W_BP + 1), word(TB_W_BP + 2));
  const float s = KIND == TB_ENV_TENNIS ? word(TB_W_TN_SCALE) : sc.racket_scale;
  const bool ball_ok = finite3(ball);
  const bool racket_ok = finite3(com) && finite1(q.x) && finite1(q.y) && finite1(q.z) && finite1(q.w) && s > 0.0f && finite1(s);

  vec3 o = mk(cam.eye[0], cam.eye[1], cam.eye[2]);
  if (cam.follow) o = o + com;
  const bool eye_ok = finite3(o);

  // ---- the lane's ray
  const float sx = (float)(2 * px + 1 - W) / (float)W, sy = (float)(H - 2 * py - 1) / (float)H;
  vec3 d = fma3(sy, mk(cam.up[0], cam.up[1], cam.up[2]), fma3(sx, mk(cam.right[0], cam.right[1], cam.right[2]), mk(cam.fwd[0], cam.fwd[1], cam.fwd[2])));
  d = (1.0f / sqrtf(dot(d, d))) * d;

  Nearest best; best.t = INFINITY; best.n = mk(0, 0, 0); best.id = 0;
  if (eye_ok) {
    take(best, ray_box(o, d, sc.ground_half), 1);
    if (sc.flags & TB_F_NET) take(best, ray_box(o, d, sc.net_half), 2);
    if (KIND == TB_ENV_SWING) {
      const float gx = word(TB_W_SW_GOAL), gy = word(TB_W_SW_GOAL + 1);
      if (finite1(gx) && finite1(gy)) {
        Span g = span_all();
        clip_round(g, mk(o.x - gx, o.y - gy, 0.0f), d, sc.goal_radius, true);
        clip_slab(g, o.z, d.z, sc.goal_half_len, mk(0, 0, 1));
        take(best, g, 3);
      }
    }
    if (ball_ok) {
      Span b = span_all();
      clip_round(b, o - ball, d, sc.ball_radius, false);
      take(best, b, 4);
    }
    if (racket_ok) {
      const vec3 oc = o - com;
      Span bound = span_all();
      clip_round(bound, oc, d, sc.bound_radius * s, false);
      if (__any(bound.ok)) {  // wave vote: no lane of this tile can see the racket otherwise
        const vec3 ob = rotate_inv(q, oc), db = rotate_inv(q, d);
        Span r = span_all();
        clip_slab(r, ob.x, db.x, sc.half_thick * s, mk(1, 0, 0));
        for (int i = 0; i < sc.n_hull; ++i) {
          const float4 ed = hull.e[i];
          const float ny = ed.w, nz = -ed.z;
          const float num = FMA(nz, ob.z - ed.y * s, ny * (ob.y - ed.x * s)), den = FMA(nz, db.z, ny * db.y);
          if (den != 0.0f) clip(r, -num / den, den < 0.0f, mk(0.0f, ny, nz));
          else if (!(num <= 0.0f)) r.ok = false;
        }
        r.n0 = rotate(q, r.n0);
        r.n1 = rotate(q, r.n1);
        take(best, r, 5);
      }
    }
  }

  // ---- shading
  const float base[6][3] = {{135, 190, 235}, {60, 140, 80}, {235, 235, 235}, {220, 60, 50}, {230, 240, 40}, {40, 60, 200}};
  float shade = 1.0f;
  if (best.id != 0) {
    const vec3 n = (1.0f / sqrtf(dot(best.n, best.n))) * best.n;
    float ndl = dot(n, mk(cam.light[0], cam.light[1], cam.light[2]));
    ndl = ndl > 0.0f ? ndl : 0.0f;  // a NaN ends here too
    ndl = ndl < 1.0f ? ndl : 1.0f;
    shade = FMA(0.65f, ndl, 0.35f);
    if (best.id == 1 && ball_ok && ball.z > sc.ground_half[2]) {
      const float hx = FMA(best.t, d.x, o.x) - ball.x, hy = FMA(best.t, d.y, o.y) - ball.y, rr = 2.0f * sc.ball_radius;
      if (FMA(hx, hx, hy * hy) < rr * rr) shade *= 0.5f;
    }
  }
  uint32_t pk = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) v = best.id == k ? base[k][c] : v;
    pk |= (uint32_t)(int)(v * shade + 0.5f) << (8 * c);
  }

  // ---- stores: cross-lane packing first (every lane takes part), then the masked stores
  const int k4 = lx & 3;
  const uint32_t pk_next = (uint32_t)__shfl_down((int)pk, 1);
  const uint32_t colour_dw = (pk >> (8 * k4)) | (pk_next << (24 - 8 * k4));  // dword k4 < 3 of the four lanes' 12 bytes
  uint32_t id_dw = (uint32_t)best.id | ((uint32_t)__shfl_down(best.id, 1) << 8);
  id_dw |= (uint32_t)__shfl_down((int)id_dw, 2) << 16;
  if (px < W && py < H) {
    const size_t pix = ((size_t)img * (size_t)H + (size_t)py) * (size_t)W + (size_t)px;
    const bool quads = (W & 3) == 0;  // then a group of four lanes is wholly inside the image and starts on a multiple of 4 pixels
    if (quads && (reinterpret_cast<uintptr_t>(rgb) & 3) == 0) {
      if (k4 < 3) *reinterpret_cast<uint32_t*>(rgb + (pix - (size_t)k4) * 3 + 4 * (size_t)k4) = colour_dw;
    } else {
      rgb[pix * 3] = (uint8_t)(pk & 255); rgb[pix * 3 + 1] = (uint8_t)((pk >> 8) & 255); rgb[pix * 3 + 2] = (uint8_t)(pk >> 16);
    }
    if (ids) {
      if (quads && (reinterpret_cast<uintptr_t>(ids) & 3) == 0) { if (k4 == 0) *reinterpret_cast<uint32_t*>(ids + pix) = id_dw; }
      else ids[pix] = (uint8_t)best.id;
    }
    if (depth) depth[pix] = best.t;
  }
}

}  // namespace tb
