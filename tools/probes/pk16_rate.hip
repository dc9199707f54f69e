// Probe: issue rate of the packed 16-bit integer instructions of the strip kernel's quick reject (csrc/fast_reject_dev.h) beside the
// 32-bit forms they replace.  Every wavefront runs n trips of 32 instructions of one kind in 8 INDEPENDENT chains; one wavefront per SIMD (256
// threads) and four (1024 threads).  Printed: clock64 ticks per instruction and wavefront, and the ratio to plain v_max_u32 -- 1.00
// means the same rate.  hipcc --offload-arch=gfx950 -O3 pk16_rate.hip -o pk16_rate && ./pk16_rate
#include <hip/hip_runtime.h>
#include <cstdio>

#define OP8(op, tail) \
  asm volatile(op " %0, %0, %8" tail "\n " op " %1, %1, %8" tail "\n " op " %2, %2, %8" tail "\n " op " %3, %3, %8" tail "\n " \
               op " %4, %4, %8" tail "\n " op " %5, %5, %8" tail "\n " op " %6, %6, %8" tail "\n " op " %7, %7, %8" tail \
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]) : "v"(b))

#define R4(x) x x x x

__global__ __launch_bounds__(1024) void k(unsigned* out, unsigned long long* cyc, int n, int mode) {
  unsigned r[8];
  for (int j = 0; j < 8; j++) r[j] = out[threadIdx.x + 1024 * j];
  const unsigned b = out[threadIdx.x ^ 1], sel = 0x0c020c00u;
  __syncthreads();
  const unsigned long long t0 = clock64();
  for (int i = 0; i < n; i++) {
    switch (mode) {
      case 0: R4(OP8("v_max_u32", "");) break;
      case 1: R4(OP8("v_max_u32_sdwa", " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:BYTE_2");) break;
      case 2: R4(OP8("v_pk_max_u16", "");) break;
      case 3: R4(OP8("v_pk_min_u16", "");) break;
      case 4: R4(OP8("v_pk_sub_i16", "");) break;
      case 5: R4(OP8("v_pk_max_i16", "");) break;
      default:
        R4(asm volatile("v_perm_b32 %0, %0, %8, %9\n v_perm_b32 %1, %1, %8, %9\n v_perm_b32 %2, %2, %8, %9\n v_perm_b32 %3, %3, %8, %9\n"
                     "v_perm_b32 %4, %4, %8, %9\n v_perm_b32 %5, %5, %8, %9\n v_perm_b32 %6, %6, %8, %9\n v_perm_b32 %7, %7, %8, %9"
                     : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]) : "v"(b), "v"(sel));)
    }
  }
  const unsigned long long t1 = clock64();
  if ((threadIdx.x & 63) == 0) cyc[threadIdx.x >> 6] = t1 - t0;
  unsigned s = 0;
  for (int j = 0; j < 8; j++) s += r[j];
  out[threadIdx.x] = s;
}

int main() {
  unsigned* d; unsigned long long* c;
  if (hipMalloc(&d, 8 * 1024 * 4) != hipSuccess || hipMalloc(&c, 16 * 8) != hipSuccess) { printf("no device memory\n"); return 1; }
  (void)hipMemset(d, 0x5a, 8 * 1024 * 4);
  const int n = 20000;
  static const char* name[7] = {"v_max_u32", "v_max_u32_sdwa", "v_pk_max_u16", "v_pk_min_u16", "v_pk_sub_i16", "v_pk_max_i16", "v_perm_b32"};
  for (int threads : {256, 1024}) {
    double base = 0;
    for (int mode = 0; mode < 7; mode++) {
      k<<<1, threads>>>(d, c, n, mode);
      if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 1; }
      k<<<1, threads>>>(d, c, n, mode);
      if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 1; }
      unsigned long long h[16];
      (void)hipMemcpy(h, c, sizeof(unsigned long long) * (threads / 64), hipMemcpyDeviceToHost);
      unsigned long long mx = 0;
      for (int w = 0; w < threads / 64; w++) if (h[w] > mx) mx = h[w];
      const double per = (double)mx / (32.0 * n) / (threads / 256);      // ticks per instruction of one wavefront, per SIMD
      if (mode == 0) base = per;
      printf("%d wavefront(s) per SIMD  %-16s %.4f ticks per instruction  x%.2f of v_max_u32\n", threads / 256, name[mode], per, per / base);
    }
  }
  (void)hipFree(d); (void)hipFree(c);
  return 0;
}
