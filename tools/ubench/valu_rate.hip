// VALU issue-rate micro-benchmark for gfx950: cycles per wave64 instruction of the ops K1 uses.
// Build: hipcc --offload-arch=gfx950 -O3 valu_rate.hip -o valu_rate ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

#define REP 64
#define ITERS 2000

#define KERNEL(name, decl, body)                                            \
  __global__ void name(int* out, int seed) {                                \
    decl;                                                                   \
    for (int it = 0; it < ITERS; ++it) {                                    \
      _Pragma("unroll") for (int r = 0; r < REP / 8; ++r) { body }          \
    }                                                                       \
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7; \
  }

#define DECL_I int a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3, a4 = seed + 4, a5 = seed + 5, a6 = seed + 6, a7 = seed + 7, b = threadIdx.x | 1
#define OP8(OP) OP(a0) OP(a1) OP(a2) OP(a3) OP(a4) OP(a5) OP(a6) OP(a7)

#define ADD(x) asm volatile("v_add_u32 %0, %0, %1" : "+v"(x) : "v"(b));
#define MUL24(x) asm volatile("v_mul_i32_i24 %0, %0, %1" : "+v"(x) : "v"(b));
#define MAD24(x) asm volatile("v_mad_i32_i24 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define MULLO(x) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(x) : "v"(b));
#define MULHI24(x) asm volatile("v_mul_hi_i32_i24 %0, %0, %1" : "+v"(x) : "v"(b));
#define ASHR(x) asm volatile("v_ashrrev_i32 %0, 1, %0" : "+v"(x));
#define ADD3(x) asm volatile("v_add3_u32 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define LSHLADD(x) asm volatile("v_lshl_add_u32 %0, %0, 1, %1" : "+v"(x) : "v"(b));
#define PKADD(x) asm volatile("v_pk_add_u16 %0, %0, %1" : "+v"(x) : "v"(b));
#define PKMAD(x) asm volatile("v_pk_mad_u16 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define PKMUL(x) asm volatile("v_pk_mul_lo_u16 %0, %0, %1" : "+v"(x) : "v"(b));
#define MADI16(x) asm volatile("v_mad_i32_i16 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define DOT2(x) asm volatile("v_dot2_i32_i16 %0, %0, %1, %0" : "+v"(x) : "v"(b));
#define DOT4(x) asm volatile("v_dot4_u32_u8 %0, %0, %1, %0" : "+v"(x) : "v"(b));
#define PERM(x) asm volatile("v_perm_b32 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define ALIGNBIT(x) asm volatile("v_alignbit_b32 %0, %0, %1, 16" : "+v"(x) : "v"(b));
#define FMA(x) asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define AND(x) asm volatile("v_and_b32 %0, %0, %1" : "+v"(x) : "v"(b));
#define DPPMOV(x) asm volatile("v_mov_b32_dpp %0, %0 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(x));
#define SUBSDWA(x) asm volatile("v_sub_u32_sdwa %0, %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:BYTE_0" : "+v"(x) : "v"(b));

#define MAX3(x) asm volatile("v_max3_i32 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define MAXI(x) asm volatile("v_max_i32 %0, %0, %1" : "+v"(x) : "v"(b));
#define BFE(x) asm volatile("v_bfe_u32 %0, %0, 8, 8" : "+v"(x));
#define LSHLOR(x) asm volatile("v_lshl_or_b32 %0, %0, 16, %1" : "+v"(x) : "v"(b));
#define ANDLIT(x) asm volatile("v_and_b32 %0, 0x7fff, %0" : "+v"(x));
#define CMPADDC(x) asm volatile("v_cmp_ge_i32_e32 vcc, %0, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(x) : "v"(b) : "vcc");
#define MULHISDWA(x) asm volatile("v_mul_hi_i32_i24_sdwa %0, %1, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(x) : "v"(b));
#define MULU24SDWA(x) asm volatile("v_mul_u32_u24_sdwa %0, %0, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1" : "+v"(x));
#define PKLSHR(x) asm volatile("v_pk_lshrrev_b16 %0, 1, %0" : "+v"(x));
#define ADDSDWA(x) asm volatile("v_add_u32_sdwa %0, %0, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1" : "+v"(x));
#define DPPADD(x) asm volatile("v_add_u32_dpp %0, %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(x) : "v"(b));
#define DPPROW(x) asm volatile("v_mov_b32_dpp %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(x));
#define SADU8(x) asm volatile("v_sad_u8 %0, %0, %1, %0" : "+v"(x) : "v"(b));
#define MOV(x) asm volatile("v_mov_b32 %0, %1" : "+v"(x) : "v"(b));
#define SUB(x) asm volatile("v_sub_u32 %0, %0, %1" : "+v"(x) : "v"(b));
#define LSHR(x) asm volatile("v_lshrrev_b32 %0, 1, %0" : "+v"(x));
#define MADU24(x) asm volatile("v_mad_u32_u24 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define ADDMIX(x) asm volatile("v_add_u32 %0, %0, %1\n\tv_mul_i32_i24 %0, %0, %1" : "+v"(x) : "v"(b));
#define LSHRB16(x) asm volatile("v_lshrrev_b16 %0, 1, %0" : "+v"(x));
#define ADDU16(x) asm volatile("v_add_u16 %0, %0, %1" : "+v"(x) : "v"(b));
#define MULHI32(x) asm volatile("v_mul_hi_i32 %0, %0, %1" : "+v"(x) : "v"(b));
#define DOT4I8(x) asm volatile("v_dot4_i32_i8 %0, %0, %1, %0" : "+v"(x) : "v"(b));
#define XOR(x) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(x) : "v"(b));
#define ADDSGPR(x) asm volatile("v_add_u32 %0, s4, %0" : "+v"(x));
#define CNDMASK(x) asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(x) : "v"(b));
#define DECL_H int a0 = seed | 0x64006400, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7, b = threadIdx.x | 0x64016401
#define PKMIN3H(x) asm volatile("v_pk_minimum3_f16 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define PKMINH(x) asm volatile("v_pk_min_f16 %0, %0, %1" : "+v"(x) : "v"(b));
#define PKMINI16(x) asm volatile("v_pk_min_i16 %0, %0, %1" : "+v"(x) : "v"(b));
#define PKMAXU16(x) asm volatile("v_pk_max_u16 %0, %0, %1" : "+v"(x) : "v"(b));
#define MIN3I16(x) asm volatile("v_min3_i16 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define MIN3F16(x) asm volatile("v_min3_f16 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define MIN3U32(x) asm volatile("v_min3_u32 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define MINU32(x) asm volatile("v_min_u32 %0, %0, %1" : "+v"(x) : "v"(b));
#define MINIMUM3F32(x) asm volatile("v_minimum3_f32 %0, %0, %1, %1" : "+v"(x) : "v"(b));
#define MINU16(x) asm volatile("v_min_u16 %0, %0, %1" : "+v"(x) : "v"(b));
// score arithmetic of K1 (LAB_NOTES.md "K1: score on SAD and dot2"): v_sad_u16, the 16-bit dot product in its VOP2 form
// (accumulates into its destination) and in its VOP3P form with the inline constant 0 as accumulator, and the score of
// four pixels from AB = A | B << 16 and C, as the nine instructions per pixel of the kernel before and as the seven
// after.  The chains work on four accumulators at a time, as score_row does on a lane's four pixels: in CHAIN7 the four
// dots and then the four subtractions, so that three instructions stand between a dot and the reader of its result
// (the wait states a v_dot result needs before another vector instruction may read it).  A chain counts as 9 (7) x 4
// instructions: the printed figure is cycles per instruction, times 9 (7) = cycles per pixel.
#define SADU16(x) asm volatile("v_sad_u16 %0, %0, %1, %0" : "+v"(x) : "v"(b));
#define DOT2C(x) asm volatile("v_dot2c_i32_i16 %0, %0, %1" : "+v"(x) : "v"(b));
#define DOT2Z(x) asm volatile("v_dot2_i32_i16 %0, %0, %1, 0" : "+v"(x) : "v"(b));
#define MULAB " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1\n\t"
#define TQ9(x, t, u) "v_lshrrev_b32 " t ", 1, " x "\n\tv_and_b32 " t ", 0x7fff, " t "\n\tv_lshrrev_b32 " u ", 17, " x "\n\t" \
                     "v_add_u32 " t ", " t ", " u "\n\tv_lshrrev_b32 " t ", 1, " t "\n\t"
#define SC9(x, t, u) TQ9(x, t, u) "v_mul_u32_u24_sdwa " u ", " x ", " x MULAB "v_mul_i32_i24 " x ", %12, %12\n\t" \
                     "v_mad_i32_i24 " x ", " t ", " t ", " x "\n\tv_sub_u32 " x ", " u ", " x "\n\t"
#define OP7(x, t, u) "v_and_b32 " t ", 0xfffefffe, " x "\n\tv_sad_u16 " t ", " t ", 0, 0\n\tv_lshrrev_b32 " t ", 2, " t "\n\t" \
                     "v_mul_u32_u24_sdwa " u ", " x ", " x MULAB "v_or_b32 " t ", %12, " t "\n\t"
#define CHAIN_OPS(w, x, y, z) \
  : "+v"(w), "+v"(x), "+v"(y), "+v"(z), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(u0), "=&v"(u1), "=&v"(u2), "=&v"(u3) : "v"(b)
#define CHAIN9(w, x, y, z) { int t0, t1, t2, t3, u0, u1, u2, u3; \
  asm volatile(SC9("%0", "%4", "%8") SC9("%1", "%5", "%9") SC9("%2", "%6", "%10") SC9("%3", "%7", "%11") CHAIN_OPS(w, x, y, z)); }
#define CHAIN7(w, x, y, z) { int t0, t1, t2, t3, u0, u1, u2, u3; \
  asm volatile(OP7("%0", "%4", "%8") OP7("%1", "%5", "%9") OP7("%2", "%6", "%10") OP7("%3", "%7", "%11") \
               "v_dot2_i32_i16 %4, %4, %4, 0\n\tv_dot2_i32_i16 %5, %5, %5, 0\n\t" \
               "v_dot2_i32_i16 %6, %6, %6, 0\n\tv_dot2_i32_i16 %7, %7, %7, 0\n\t" \
               "v_sub_u32 %0, %8, %4\n\tv_sub_u32 %1, %9, %5\n\tv_sub_u32 %2, %10, %6\n\tv_sub_u32 %3, %11, %7" \
               CHAIN_OPS(w, x, y, z)); }
KERNEL(k_sadu16, DECL_I, OP8(SADU16))
KERNEL(k_dot2c, DECL_I, OP8(DOT2C))
KERNEL(k_dot2z, DECL_I, OP8(DOT2Z))
KERNEL(k_score9, DECL_I, CHAIN9(a0, a1, a2, a3) CHAIN9(a4, a5, a6, a7))
KERNEL(k_score7, DECL_I, CHAIN7(a0, a1, a2, a3) CHAIN7(a4, a5, a6, a7))
// the same operations with K1's matrix instruction between them (one v_mfma_i32_4x4x4i8 per vector instruction, four
// accumulators in turn): what a dot product costs while MFMAs are in flight, against a 24-bit multiply and an add
typedef int v4i_t __attribute__((ext_vector_type(4)));
#define KERNELM(name, body)                                                 \
  __global__ void name(int* out, int seed) {                                \
    DECL_I;                                                                 \
    v4i_t m0 = {seed, 1, 2, 3}, m1 = m0, m2 = m0, m3 = m0;                  \
    int ma = threadIdx.x * 0x01010101, mb = seed * 0x01020304;              \
    asm volatile("" : "+v"(ma), "+v"(mb));                                  \
    for (int it = 0; it < ITERS; ++it) {                                    \
      _Pragma("unroll") for (int r = 0; r < REP / 8; ++r) { body }          \
    }                                                                       \
    const v4i_t m = m0 + m1 + m2 + m3;                                      \
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + m[0] + m[1] + m[2] + m[3]; \
  }
#define MF(acc) asm volatile("v_mfma_i32_4x4x4_16b_i8 %0, %1, %2, %0" : "+v"(acc) : "v"(ma), "v"(mb));
#define NOP1(x)
#define MIX8(OP) OP(a0) MF(m0) OP(a1) MF(m1) OP(a2) MF(m2) OP(a3) MF(m3) OP(a4) MF(m0) OP(a5) MF(m1) OP(a6) MF(m2) OP(a7) MF(m3)
KERNELM(k_mfma, MIX8(NOP1))
KERNELM(k_mfma_add, MIX8(ADD))
KERNELM(k_mfma_mul24, MIX8(MUL24))
KERNELM(k_mfma_mad24, MIX8(MAD24))
KERNELM(k_mfma_sadu16, MIX8(SADU16))
KERNELM(k_mfma_dot2z, MIX8(DOT2Z))
KERNELM(k_mfma_dot2c, MIX8(DOT2C))
KERNEL(k_pkmin3h, DECL_H, OP8(PKMIN3H))
KERNEL(k_pkminh, DECL_H, OP8(PKMINH))
KERNEL(k_pkmini16, DECL_H, OP8(PKMINI16))
KERNEL(k_pkmaxu16, DECL_H, OP8(PKMAXU16))
KERNEL(k_min3i16, DECL_H, OP8(MIN3I16))
KERNEL(k_min3f16, DECL_H, OP8(MIN3F16))
KERNEL(k_min3u32, DECL_H, OP8(MIN3U32))
KERNEL(k_minu32, DECL_H, OP8(MINU32))
KERNEL(k_minimum3f32, DECL_H, OP8(MINIMUM3F32))
KERNEL(k_minu16, DECL_H, OP8(MINU16))
KERNEL(k_lshrb16, DECL_I, OP8(LSHRB16))
KERNEL(k_addu16, DECL_I, OP8(ADDU16))
KERNEL(k_mulhi32, DECL_I, OP8(MULHI32))
KERNEL(k_dot4i8, DECL_I, OP8(DOT4I8))
KERNEL(k_xor, DECL_I, OP8(XOR))
KERNEL(k_cndmask, DECL_I, OP8(CNDMASK))
KERNEL(k_max3, DECL_I, OP8(MAX3))
KERNEL(k_maxi, DECL_I, OP8(MAXI))
KERNEL(k_bfe, DECL_I, OP8(BFE))
KERNEL(k_lshlor, DECL_I, OP8(LSHLOR))
KERNEL(k_andlit, DECL_I, OP8(ANDLIT))
KERNEL(k_cmpaddc2, DECL_I, OP8(CMPADDC))
KERNEL(k_mulhisdwa, DECL_I, OP8(MULHISDWA))
KERNEL(k_mulu24sdwa, DECL_I, OP8(MULU24SDWA))
KERNEL(k_pklshr, DECL_I, OP8(PKLSHR))
KERNEL(k_addsdwa, DECL_I, OP8(ADDSDWA))
KERNEL(k_dppadd, DECL_I, OP8(DPPADD))
KERNEL(k_dpprow, DECL_I, OP8(DPPROW))
KERNEL(k_sadu8, DECL_I, OP8(SADU8))
KERNEL(k_mov, DECL_I, OP8(MOV))
KERNEL(k_sub, DECL_I, OP8(SUB))
KERNEL(k_lshr, DECL_I, OP8(LSHR))
KERNEL(k_madu24, DECL_I, OP8(MADU24))
KERNEL(k_addmul2, DECL_I, OP8(ADDMIX))
KERNEL(k_add, DECL_I, OP8(ADD))
KERNEL(k_mul24, DECL_I, OP8(MUL24))
KERNEL(k_mad24, DECL_I, OP8(MAD24))
KERNEL(k_mullo, DECL_I, OP8(MULLO))
KERNEL(k_mulhi24, DECL_I, OP8(MULHI24))
KERNEL(k_ashr, DECL_I, OP8(ASHR))
KERNEL(k_add3, DECL_I, OP8(ADD3))
KERNEL(k_lshladd, DECL_I, OP8(LSHLADD))
KERNEL(k_pkadd, DECL_I, OP8(PKADD))
KERNEL(k_pkmad, DECL_I, OP8(PKMAD))
KERNEL(k_pkmul, DECL_I, OP8(PKMUL))
KERNEL(k_madi16, DECL_I, OP8(MADI16))
KERNEL(k_dot2, DECL_I, OP8(DOT2))
KERNEL(k_dot4, DECL_I, OP8(DOT4))
KERNEL(k_perm, DECL_I, OP8(PERM))
KERNEL(k_alignbit, DECL_I, OP8(ALIGNBIT))
KERNEL(k_fma, DECL_I, OP8(FMA))
KERNEL(k_and, DECL_I, OP8(AND))
KERNEL(k_dppmov, DECL_I, OP8(DPPMOV))
KERNEL(k_subsdwa, DECL_I, OP8(SUBSDWA))

int main() {
  int* d;
  const int blocks = 256 * 8, threads = 256;  // 8 waves per SIMD
  hipMalloc(&d, blocks * threads * sizeof(int));
  hipDeviceProp_t p;
  hipGetDeviceProperties(&p, 0);
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
#define RUN(k) RUNN(k, 1)
#define RUNN(k, N)                                                                          \
  {                                                                                         \
    k<<<blocks, threads>>>(d, 1);                                                           \
    hipDeviceSynchronize();                                                                 \
    hipEventRecord(a);                                                                      \
    k<<<blocks, threads>>>(d, 1);                                                           \
    hipEventRecord(b);                                                                      \
    hipEventSynchronize(b);                                                                 \
    float ms;                                                                               \
    hipEventElapsedTime(&ms, a, b);                                                         \
    const double instr = (double)blocks * (threads / 64) * ITERS * REP * (N);                   \
    const double per_simd = instr / (p.multiProcessorCount * 4);                            \
    printf("%-10s %.3f ms  -> %.2f ns per wave-instr per SIMD (= %.2f cycles @2.4GHz)\n", #k, ms, \
           ms * 1e6 / per_simd, ms * 1e6 / per_simd * 2.4);                                 \
  }
  RUN(k_add) RUN(k_mul24) RUN(k_mad24) RUN(k_mullo) RUN(k_mulhi24) RUN(k_ashr) RUN(k_add3) RUN(k_lshladd)
  RUN(k_pkadd) RUN(k_pkmad) RUN(k_pkmul) RUN(k_madi16) RUN(k_dot2) RUN(k_dot4) RUN(k_perm) RUN(k_alignbit)
  RUN(k_fma) RUN(k_and) RUN(k_dppmov) RUN(k_subsdwa)
  printf("-- round 2 additions (k_cmpaddc2 and k_addmul2 are TWO instructions per count)\n");
  RUN(k_max3) RUN(k_maxi) RUN(k_bfe) RUN(k_lshlor) RUN(k_andlit) RUN(k_cmpaddc2) RUN(k_mulhisdwa)
  RUN(k_mulu24sdwa) RUN(k_pklshr) RUN(k_addsdwa) RUN(k_dppadd) RUN(k_dpprow) RUN(k_sadu8) RUN(k_mov)
  RUN(k_sub) RUN(k_lshr) RUN(k_madu24) RUN(k_addmul2)
  RUN(k_lshrb16) RUN(k_addu16) RUN(k_mulhi32) RUN(k_dot4i8) RUN(k_xor) RUN(k_cndmask)
  printf("-- round 4: minima / maxima (AGAST kernel)\n");
  RUN(k_pkmin3h) RUN(k_pkminh) RUN(k_pkmini16) RUN(k_pkmaxu16) RUN(k_min3i16) RUN(k_min3f16) RUN(k_min3u32)
  RUN(k_minu32) RUN(k_minimum3f32) RUN(k_minu16)
  printf("-- K1 score arithmetic (k_score9 / k_score7: per instruction of the 9- / 7-instruction chain per pixel)\n");
  RUN(k_sadu16) RUN(k_dot2c) RUN(k_dot2z) RUNN(k_score9, 9) RUNN(k_score7, 7)
  printf("-- one v_mfma_i32_4x4x4i8 per vector instruction (figures per PAIR; k_mfma: the MFMA alone)\n");
  RUN(k_mfma) RUN(k_mfma_add) RUN(k_mfma_mul24) RUN(k_mfma_mad24) RUN(k_mfma_sadu16) RUN(k_mfma_dot2z) RUN(k_mfma_dot2c)
  return 0;
}
