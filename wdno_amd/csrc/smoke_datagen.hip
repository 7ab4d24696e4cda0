// smoke_datagen.hip -- the smoke training-set simulator (smoke/dataset/a_gen_train.py:363-456, 502-696 and its a_gen_test_64 / a_gen_test_128
// twins) as ONE launch: one workgroup per scene runs frames 0..scenelength, each with the same steps as the control-evaluation solver
// (smoke_solver.hip) -- compose the velocity, mask it, divergence, CG pressure solve, projection, advection of the two densities -- which
// both kernels take from smoke_flow.h. What is the generator's own:
//
//   rim      there is no control input. On an ordinary frame the 16-cell rim is the previous frame's projected rim plus N(0, 0.1) noise
//            (a random walk), fp32(fp64(previous) + noise); on the four kick frames of a scene it is a fresh field N(v, |v| / 10), fp32(noise).
//            The noise is either read (explicit source: float64 [B][scenelength + 1][128][128][2], what np.random.normal delivered; only rim
//            cells are read) or made in the kernel (seeded source: Philox4x32-10 + Box-Muller in fp32, below). The seeded source IS the
//            explicit one fed with its own fp32 fields widened to fp64: from the noise value on, one code path.
//   buckets  the rule tests and zeroes the set-zero density; it sums on the recorded stride; on a kick frame it runs only if the frame is
//            recorded; at frame 0 it never runs.
//   records  every record_scale-th frame at spatial stride 1 or 2: density (the density that is never zeroed), velocity, control (the rim
//            field before the velocity mask, interior 0) in fp32 and smoke [8] in fp64: the seven bucket totals and column 7, a sum over
//            the strided cells of the set-zero density after zeroing (ordinary frame) or of the density (kick frame, frame 0).
//            Record 0 of the velocity holds component 0 in both slots, as the reference writes it (a_gen_train.py:453-454).
//   advect   the advection coordinate idx - v is formed in fp64 from the fp32 centred velocity (sm_advect_cell<true>); the solver keeps the
//            reference's fp32 difference. Near idx = 100 that difference is off by up to 3.8e-6 cells per frame, which moved a front's
//            leading edge -- the first smoke in a bucket -- by ~1e-5 relative; in fp64 the term is gone.
//   frame 0  the densities of frame 0 are the one initial density advected once: both planes start equal, so both advections give the same bits.
//
// The rim composition and the random numbers live in the rolled per-frame part, outside the CG loop.
#include "smoke_flow.h"

namespace {

using namespace smoke;

constexpr int NQG = 11;     // per-frame sums: 7 buckets (strided cells), the union (all cells), and on the strided cells the density, the set-zero density before / after the bucket mask

struct GenP {
  const int* scene_i;               // [B][8]: xs0, ys0, the four kick frames, 0, 0
  const float* scene_v;             // [B][8]: (vx, vy) of the four kicks
  const long long* scene_index;     // [B]: the scene's number in the data set (the seeded source's counter)
  const double* noise;              // explicit source, or null
  const float* v0;
  const float* fluid; const float* active; const float* vmask; const float* buckets;
  float* dens; float* vel; float* ctrl; double* smoke; float* ws;
  unsigned long long seed;
  int S, rs, stride, R, nrec, max_iter;
  float accuracy;
};

// ---- the seeded noise source: Philox4x32-10 (Salmon et al., SC'11), key = the data set's 64-bit seed, counter = (cell, frame, scene lo, scene hi)
__device__ __forceinline__ uint4 sm_philox(uint4 c, uint2 k) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x, hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += W0; k.y += W1;
  }
  return c;
}

// two unit normals of cell c of a frame of a scene: u = ((x >> 9) + 0.5) 2^-23 in [2^-24, 1 - 2^-24], exact in fp32; Box-Muller in fp32
__device__ __forceinline__ float2 sm_unit_normals(unsigned long long seed, long long scene, int frame, int c) {
  const uint4 x = sm_philox(make_uint4((unsigned)c, (unsigned)frame, (unsigned)((unsigned long long)scene & 0xffffffffu), (unsigned)((unsigned long long)scene >> 32)),
                            make_uint2((unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32)));
  const float u1 = __fmul_rn(__fadd_rn((float)(x.x >> 9), 0.5f), 1.1920928955078125e-07f);
  const float u2 = __fmul_rn(__fadd_rn((float)(x.y >> 9), 0.5f), 1.1920928955078125e-07f);
  const float r = sqrtf(__fmul_rn(-2.f, logf(u1)));
  float sn, cs;
  sincospif(__fmul_rn(2.f, u2), &sn, &cs);            // the angle 2 pi u2: 2 u2 is exact, the reduction is done on it
  return make_float2(__fmul_rn(r, cs), __fmul_rn(r, sn));
}

// the field the seeded source delivers: 0.1 z on an ordinary frame, v + (|v| / 10) z on a kick
__device__ __forceinline__ float2 sm_noise_field(unsigned long long seed, long long scene, int frame, int c, bool kick, float vx, float vy) {
  const float2 z = sm_unit_normals(seed, scene, frame, c);
  if (!kick) return make_float2(__fmul_rn(0.1f, z.x), __fmul_rn(0.1f, z.y));
  return make_float2(__fadd_rn(vx, __fmul_rn(__fdiv_rn(fabsf(vx), 10.f), z.x)), __fadd_rn(vy, __fmul_rn(__fdiv_rn(fabsf(vy), 10.f), z.y)));
}

// A copy of a lane's column that the compiler cannot see through: what a per-frame stage derives from it (addresses, record offsets, stride
// tests) is computed inside that stage and is not kept in registers across the CG loop, which runs at the register limit.
__device__ __forceinline__ int sm_stage_col(int col0) {
  asm volatile("" : "+v"(col0));
  return col0;
}

template <int NT>
__global__ __launch_bounds__(NT) void smoke_generate_kernel(GenP P) {
  constexpr int NW = NT / 64;          // waves
  constexpr int RR = SG / NW;          // rows per wave: 8 or 16
  constexpr int NGW = RR / 8;          // reduction groups per wave
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = w * RR, col0 = 2 * lane;
  const size_t n = blockIdx.x;

  __shared__ SmShared<NW, NQG> sh;
  if (threadIdx.x < 7) sh.outs[threadIdx.x] = 0.0;

  const SmWorkspace W = sm_workspace(P.ws, n);
  float2* __restrict__ velws = W.vel;
  const float2* __restrict__ vmask = reinterpret_cast<const float2*>(P.vmask);
  const int* __restrict__ sci = P.scene_i + n * 8;
  const float* __restrict__ scv = P.scene_v + n * 8;
  const long long scene = P.scene_index[n];
  const int st = P.stride, nrec = P.nrec;
  const size_t rcells = (size_t)nrec * nrec;
  float* __restrict__ odens = P.dens + n * P.R * rcells;
  float2* __restrict__ ovel = reinterpret_cast<float2*>(P.vel) + n * P.R * rcells;
  float2* __restrict__ octrl = reinterpret_cast<float2*>(P.ctrl) + n * P.R * rcells;
  double* __restrict__ osmoke = P.smoke + n * P.R * 8;

  float dg[RR][2];
  bool act[RR][2];
  sm_stencil<RR>(P.fluid, P.active, row0, col0, dg, act);

  // initial state: velocity, the 11 x 11 block of density in both planes of buffer 0 (row / column 127 are zero in every buffer)
  {
    const int xs0 = sci[0], ys0 = sci[1];
    const float2* __restrict__ v0 = reinterpret_cast<const float2*>(P.v0);
#pragma unroll 1
    for (int k = 0; k < RR; ++k)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = row0 + k, j = col0 + e, c = i * SG + j;
        velws[c] = v0[c];
        const float d = (i < SN && j < SN && i >= ys0 && i < ys0 + 11 && j >= xs0 && j < xs0 + 11) ? 1.f : 0.f;
        W.dbuf0[c] = d; W.dbuf0[SCELLS + c] = d;
        W.dbuf1[c] = 0.f; W.dbuf1[SCELLS + c] = 0.f;
      }
  }
  __syncthreads();

#pragma unroll 1
  for (int frame = 0; frame <= P.S; ++frame) {
    int kick = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) kick = sci[2 + k] == frame ? k : kick;
    const bool is_kick = kick >= 0, rec = frame % P.rs == 0;
    const size_t obase = (size_t)(frame / P.rs) * rcells;               // used on record frames only
    const float kvx = is_kick ? scv[2 * kick] : 0.f, kvy = is_kick ? scv[2 * kick + 1] : 0.f;

    // ---- the frame's velocity: interior from the previous frame, rim from the random walk or the kick; the control record; masked
    {
      const int colc = sm_stage_col(col0);
      const double* __restrict__ nz = P.noise ? P.noise + (n * (size_t)(P.S + 1) + frame) * (size_t)(2 * SCELLS) : nullptr;
#pragma unroll 1
      for (int k = 0; k < RR; ++k)
#pragma unroll 1
        for (int e = 0; e < 2; ++e) {
          const int i = row0 + k, j = colc + e, c = i * SG + j;
          float2 v = velws[c], cr = make_float2(0.f, 0.f);
          if (!sm_interior(i, j)) {
            double nx, ny;
            if (nz) {
              nx = nz[2 * c]; ny = nz[2 * c + 1];
            } else {
              const float2 f = sm_noise_field(P.seed, scene, frame, c, is_kick, kvx, kvy);
              nx = (double)f.x; ny = (double)f.y;
            }
            if (is_kick) v = make_float2((float)nx, (float)ny);
            else v = make_float2((float)((double)v.x + nx), (float)((double)v.y + ny));
            cr = v;
          }
          if (rec && i % st == 0 && j % st == 0) octrl[obase + (size_t)(i / st) * nrec + j / st] = cr;
          const float2 m = vmask[c];
          velws[c] = make_float2(__fmul_rn(v.x, m.x), __fmul_rn(v.y, m.y));
        }
    }
    __syncthreads();

    // ---- divergence, CG, pressure to the workspace, then the projection and the velocity record
    sm_divergence<RR>(W, row0, sm_stage_col(col0));
    sm_pressure_solve<NT, NQG>(sh, dg, act, W, P.max_iter, P.accuracy, lane, w, row0, col0);
    __syncthreads();
    sm_project<RR>(W, vmask, row0, sm_stage_col(col0), [&](int i, int j, int, float2 v) {
      if (rec && i % st == 0 && j % st == 0) ovel[obase + (size_t)(i / st) * nrec + j / st] = frame == 0 ? make_float2(v.x, v.x) : v;
    });
    __syncthreads();

    // ---- advection of both densities, the density record and the per-frame sums
    const float* __restrict__ src = W.buffer(frame & 1);
    float* __restrict__ dst = W.buffer((frame & 1) ^ 1);
    const int cola = sm_stage_col(col0);
#pragma unroll 1
    for (int g = 0; g < NGW; ++g) {
      double s[NQG];
#pragma unroll
      for (int qn = 0; qn < NQG; ++qn) s[qn] = 0.0;
#pragma unroll 1
      for (int kk = 0; kk < 8; ++kk)
#pragma unroll 1
        for (int e = 0; e < 2; ++e) {
          const int i = row0 + g * 8 + kk, j = cola + e, c = i * SG + j;
          float d, z;
          sm_advect_cell<true>(velws, src, i, j, c, d, z);
          dst[c] = d;
          dst[SCELLS + c] = z;
          const bool on = i % st == 0 && j % st == 0;                  // a recorded cell
          if (rec && on) odens[obase + (size_t)(i / st) * nrec + j / st] = d;
          bool any = false;
#pragma unroll
          for (int b = 0; b < 7; ++b) {
            const float bm = P.buckets[b * SCELLS + c];
            s[b] += on ? (double)z * (double)bm : 0.0;
            any = any || bm != 0.f;
          }
          s[7] += any ? (double)z : 0.0;
          s[8] += on ? (double)d : 0.0;
          s[9] += on ? (double)z : 0.0;
          s[10] += on ? (double)z * (double)P.buckets[7 * SCELLS + c] : 0.0;
        }
      sm_group_sums<NQG, NW>(sh, s, lane, w * NGW + g);
    }
    __syncthreads();
    // the bucket rule: every ordinary frame after frame 0; a kick frame only when it is recorded (a_gen_train.py:562-565, 581-584, 514-517)
    double in_buckets = 0.0;
#pragma unroll
    for (int g = 0; g < NGROUP; ++g) in_buckets += sh.fred[7][g];
    const bool hit = frame > 0 && (!is_kick || rec) && in_buckets > 0.0;
    if (hit) {
#pragma unroll 1
      for (int k = 0; k < RR; ++k)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int c = (row0 + k) * SG + cola + e;                    // own cells: written above by this thread
          dst[SCELLS + c] = __fmul_rn(dst[SCELLS + c], P.buckets[7 * SCELLS + c]);
        }
    }
    if (threadIdx.x == 0) {
      if (hit)
        for (int b = 0; b < 7; ++b) {
          double sb = 0.0;
          for (int g = 0; g < NGROUP; ++g) sb += sh.fred[b][g];
          sh.outs[b] += sb;
        }
      if (rec) {
        double* __restrict__ o = osmoke + (size_t)(frame / P.rs) * 8;
        for (int b = 0; b < 7; ++b) o[b] = sh.outs[b];
        const int q = (frame == 0 || is_kick) ? 8 : (hit ? 10 : 9);    // column 7: a_gen_train.py:544, 520, 574
        double t = 0.0;
        for (int g = 0; g < NGROUP; ++g) t += sh.fred[q][g];
        o[7] = t;
      }
    }
    __syncthreads();
  }
}

// the fields the seeded source delivers for item blockIdx.y: scene_index, frame, kick flag and (vx, vy) per item
__global__ __launch_bounds__(256) void smoke_noise_kernel(const long long* __restrict__ scene_index, const int* __restrict__ frame,
                                                          const int* __restrict__ is_kick, const float* __restrict__ kick_v,
                                                          unsigned long long seed, float2* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;                         // grid.x = SCELLS / 256
  const size_t it = blockIdx.y;
  out[it * SCELLS + c] = sm_noise_field(seed, scene_index[it], frame[it], c, is_kick[it] != 0, kick_v[2 * it], kick_v[2 * it + 1]);
}

template <int NT>
int gen_launch(const GenP& p, int B, hipStream_t st) {
  smoke_generate_kernel<NT><<<B, NT, 0, st>>>(p);
  return wdno_check_launch();
}

}  // namespace

extern "C" int wdno_smoke_generate(const int* scene_i, const float* scene_v, const long long* scene_index, const double* noise,
                                   const float* init_velocity, const float* fluid_ext, const float* active_ext, const float* velocity_mask,
                                   const float* buckets, float* density, float* velocity, float* control, double* smoke, float* ws,
                                   const wdno_smoke_generate_desc* d, wdno_stream_t s) {
  WDNO_REQUIRE(scene_i && scene_v && scene_index && init_velocity && fluid_ext && active_ext && velocity_mask && buckets && density && velocity &&
               control && smoke && ws && d);
  WDNO_REQUIRE(d->B > 0 && d->scenelength >= 1 && d->scenelength <= 256 && d->record_scale >= 1 && (d->stride == 1 || d->stride == 2));
  WDNO_REQUIRE(d->max_iter >= 0 && d->max_iter <= 500);
  WDNO_REQUIRE((d->noise_mode == 0) == (noise != nullptr) && (d->noise_mode == 0 || d->noise_mode == 1));
  GenP p;
  p.scene_i = scene_i; p.scene_v = scene_v; p.scene_index = scene_index; p.noise = noise; p.v0 = init_velocity;
  p.fluid = fluid_ext; p.active = active_ext; p.vmask = velocity_mask; p.buckets = buckets;
  p.dens = density; p.vel = velocity; p.ctrl = control; p.smoke = smoke; p.ws = ws;
  p.seed = d->seed;
  p.S = d->scenelength; p.rs = d->record_scale; p.stride = d->stride; p.R = d->scenelength / d->record_scale + 1; p.nrec = SG / d->stride;
  p.max_iter = d->max_iter; p.accuracy = d->accuracy;
  hipStream_t st = as_stream(s);
  switch (d->threads) {
    case 1024: return gen_launch<1024>(p, d->B, st);
    case 512: return gen_launch<512>(p, d->B, st);
  }
  return WDNO_EUNSUPPORTED;
}

extern "C" int wdno_smoke_noise(const long long* scene_index, const int* frame, const int* is_kick, const float* kick_v, int n,
                                unsigned long long seed, float* out, wdno_stream_t s) {
  WDNO_REQUIRE(scene_index && frame && is_kick && kick_v && out && n > 0 && n <= 65535);
  smoke_noise_kernel<<<dim3(SCELLS / 256, n), 256, 0, as_stream(s)>>>(scene_index, frame, is_kick, kick_v, seed,
                                                                      reinterpret_cast<float2*>(out));
  return wdno_check_launch();
}
