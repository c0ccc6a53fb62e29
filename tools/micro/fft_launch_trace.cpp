// Host-side launch trace of the FFT convolution's entry points (no GPU needed): loads a libeqa_hip.so, answers the HIP runtime
// calls of its launch code itself and prints, for every case, the status and every launch -- kernel, grid, block, dynamic LDS and
// the low 32 bits of each argument.  Two libraries that print the same text launch the same kernels the same way.
//   fft_launch_trace LIB.so SYMBOLS   (SYMBOLS: `offset nargs name` per kernel; tools/fft_launch_trace.py builds it and runs this)
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <map>
#include <string>
struct dim3_ { unsigned x, y, z; };
static std::map<uintptr_t, std::pair<int, std::string>> g_sym;  // offset -> (nargs, name)
static uintptr_t g_base;
static const char* g_case = "";
extern "C" {
int hipLaunchKernel(const void* f, dim3_ g, dim3_ b, void** args, size_t shmem, void* st) {
  auto it = g_sym.find((uintptr_t)f - g_base);
  if (it == g_sym.end()) { printf("%s | UNKNOWN %p\n", g_case, f); return 0; }
  printf("%s | %s grid=%u,%u,%u block=%u,%u,%u lds=%zu args=", g_case, it->second.second.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, shmem);
  for (int i = 0; i < it->second.first; ++i) printf("%08x ", *(unsigned*)args[i]);
  printf("\n");
  return 0;
}
static dim3_ cg, cb; static size_t cs_; static void* cst;
int __hipPushCallConfiguration(dim3_ g, dim3_ b, size_t s, void* st) { cg = g; cb = b; cs_ = s; cst = st; return 0; }
int __hipPopCallConfiguration(dim3_* g, dim3_* b, size_t* s, void** st) { *g = cg; *b = cb; *s = cs_; *st = cst; return 0; }
int hipGetLastError() { return 0; }
int hipGetDevice(int* d) { *d = 0; return 0; }
int hipFuncSetAttribute(const void*, int, int) { return 0; }
int hipDeviceGetAttribute(int* v, int, int) { *v = 256; return 0; }
}
typedef int (*fn_t)(...);
int main(int argc, char** argv) {
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  Dl_info di; dladdr(dlsym(h, "eqa_abi_version"), &di); g_base = (uintptr_t)di.dli_fbase;
  FILE* f = fopen(argv[2], "r"); char name[4096]; unsigned long off; int n;
  while (fscanf(f, "%lx %d %4095s", &off, &n, name) == 3) g_sym[off] = {n, name};
  auto F = [&](const char* s) { return (fn_t)dlsym(h, s); };
  void *A = (void*)0x10000, *B = (void*)0x20000, *C_ = (void*)0x30000, *D = (void*)0x40000, *E = (void*)0x50000;
  char cs[256];
  const int maps[][2] = {{92, 92}, {53, 50}, {20, 33}, {137, 49}, {15, 50}, {11, 50}, {56, 56}, {60, 97}};
  for (int pipe = 0; pipe < 2; ++pipe) {
    if (pipe) setenv("EQA_FFT_FWD_PIPE", "1", 1);
    for (int nimg : {2, 25, 128}) for (int Cc : {8, 16, 24, 48, 64}) for (auto& m : maps) {
      const int H = m[0], W = m[1];
      for (int act = 0; act < 2; ++act) {
        snprintf(cs, sizeof cs, "pipe=%d n=%d C=%d %dx%d act=%d k5_input", pipe, nimg, Cc, H, W, act); g_case = cs;
        printf("%s -> %d\n", cs, F("eqa_fft48k5_input")(A, B, C_, act ? D : nullptr, act, nimg, H, W, Cc, nullptr));
        snprintf(cs, sizeof cs, "pipe=%d n=%d C=%d %dx%d act=%d k5_input_grouped", pipe, nimg, Cc, H, W, act); g_case = cs;
        printf("%s -> %d\n", cs, F("eqa_fft48k5_input_grouped")(A, B, C_, act ? D : nullptr, act, nimg, H, W, Cc, nullptr));
        if (pipe) continue;
        snprintf(cs, sizeof cs, "n=%d C=%d %dx%d act=%d k5_output", nimg, Cc, H, W, act); g_case = cs;
        printf("%s -> %d\n", cs, F("eqa_fft48k5_output")(A, B, act ? D : nullptr, act, C_, nimg, H, W, Cc, nullptr));
        for (int kn : {3, 5, 4}) {
          snprintf(cs, sizeof cs, "n=%d C=%d %dx%d act=%d k_next=%d k5_output_sums", nimg, Cc, H, W, act, kn); g_case = cs;
          printf("%s -> %d\n", cs, F("eqa_fft48k5_output_sums")(A, B, act ? D : nullptr, act, C_, E, nimg, H, W, Cc, kn, nullptr));
        }
        for (int k : {3, 5, 7, 9}) {
          snprintf(cs, sizeof cs, "n=%d C=%d %dx%d act=%d k=%d any_input", nimg, Cc, H, W, act, k); g_case = cs;
          printf("%s -> %d\n", cs, F("eqa_fft48_input")(A, B, C_, act ? D : nullptr, act, nimg, H, W, Cc, k, nullptr));
          snprintf(cs, sizeof cs, "n=%d C=%d %dx%d act=%d k=%d any_output", nimg, Cc, H, W, act, k); g_case = cs;
          printf("%s -> %d\n", cs, F("eqa_fft48_output")(A, B, act ? D : nullptr, act, C_, nimg, H, W, Cc, k, nullptr));
        }
      }
      if (pipe) continue;
      snprintf(cs, sizeof cs, "n=%d C=%d %dx%d k5_grad_transform", nimg, Cc, H, W); g_case = cs;
      printf("%s -> %d\n", cs, F("eqa_fft48k5_grad_transform")(A, B, C_, nimg, H, W, Cc, nullptr));
      snprintf(cs, sizeof cs, "n=%d C=%d %dx%d k5_input_grad", nimg, Cc, H, W); g_case = cs;
      printf("%s -> %d\n", cs, F("eqa_fft48k5_input_grad")(A, B, C_, nimg, H, W, Cc, nullptr));
      snprintf(cs, sizeof cs, "n=%d C=%d %dx%d k5_output_stats", nimg, Cc, H, W); g_case = cs;
      printf("%s -> %d rows=%ld\n", cs, F("eqa_fft48k5_output_stats")(A, B, C_, D, nimg, H, W, Cc, nullptr),
             ((long (*)(int, int, int, int))dlsym(h, "eqa_fft48k5_output_stats_rows"))(nimg, H, W, Cc));
      printf("%s ws=%ld\n", cs, ((long (*)(int, int, int, int))dlsym(h, "eqa_fft48k5_workspace_bytes"))(nimg, H, W, Cc));
      for (int k : {3, 5, 7, 9}) {
        snprintf(cs, sizeof cs, "n=%d C=%d %dx%d k=%d any_grad_transform", nimg, Cc, H, W, k); g_case = cs;
        printf("%s -> %d\n", cs, F("eqa_fft48_grad_transform")(A, B, C_, nimg, H, W, Cc, k, nullptr));
        snprintf(cs, sizeof cs, "n=%d C=%d %dx%d k=%d any_input_grad", nimg, Cc, H, W, k); g_case = cs;
        printf("%s -> %d\n", cs, F("eqa_fft48_input_grad")(A, B, C_, nimg, H, W, Cc, k, nullptr));
        printf("%s ws=%ld tiles=%ld\n", cs, ((long (*)(int, int, int, int, int))dlsym(h, "eqa_fft48_workspace_bytes"))(nimg, H, W, Cc, k),
               ((long (*)(int, int))dlsym(h, "eqa_fft48_tiles"))(H, k));
      }
    }
  }
  const int ch[][2] = {{8, 12}, {64, 64}, {512, 16}, {32, 64}, {70000, 16}, {16, 600}};
  for (auto& c : ch) for (int corr = 0; corr < 2; ++corr) {
    const int Cin = c[0], Cout = c[1];
    snprintf(cs, sizeof cs, "Cin=%d Cout=%d x=%d k5_filter", Cin, Cout, corr); g_case = cs;
    printf("%s -> %d %d %d %d\n", cs, F("eqa_fft48k5_filter_spectra")(A, B, Cout, Cin, corr, nullptr), F("eqa_fft48k5_filter_spectra3m")(A, B, Cout, Cin, corr, nullptr),
           F("eqa_fft48k5_filter_grad")(A, B, Cout, Cin, nullptr), F("eqa_fft48k5_filter_grad3m")(A, B, Cout, Cin, nullptr));
    for (int k : {3, 5, 7, 9, 4}) {
      snprintf(cs, sizeof cs, "Cin=%d Cout=%d x=%d k=%d any_filter", Cin, Cout, corr, k); g_case = cs;
      printf("%s -> %d %d %d\n", cs, F("eqa_fft48_filter_spectra")(A, B, Cout, Cin, k, corr, nullptr), F("eqa_fft48_filter_spectra3m")(A, B, Cout, Cin, k, corr, nullptr),
             F("eqa_fft48_filter_grad")(A, B, Cout, Cin, k, corr, nullptr));
    }
  }
  return 0;
}
