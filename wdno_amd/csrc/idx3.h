// idx3.h -- a flat index split three ways once and then advanced by additions: the loops of csrc/smoke_reconstruct.hip and csrc/smoke_score.hip
// walk idx = (c * B + b) * A + a in steps of the workgroup size without an integer division per element.
#pragma once

template <int STEP>
struct Idx3 {
  int a, b, c, A, B, da, db, dc;
  __device__ __forceinline__ Idx3(int tid, int A_, int B_) : A(A_), B(B_) {      // tid < STEP
    a = tid % A; int t = tid / A; b = t % B; c = t / B;
    da = STEP % A; t = STEP / A; db = t % B; dc = t / B;
  }
  __device__ __forceinline__ void next() {
    a += da; if (a >= A) { a -= A; ++b; }
    b += db; if (b >= B) { b -= B; ++c; }
    c += dc;
  }
};
