// rollout_plugin.hip -- the fused roll-out for dimension sets without a built-in instantiation (host code only).
//
// The reference's dimensions are constants edited in its scripts (duffing.py:66 Nlift, :632-633 MPCHorizon; the MATLAB twin runs
// L = 10, N = 10: Koopman_update.m:67, 70, 113).  libkoopmpc.so carries rollout_kernel<L, N, q, ...> for the sets BASELINE.json and
// the reference's scripts use; for any other set the kernel is made when a handle of that set is created (kmpc_create,
// kmpc_set_terminal_refresh, kmpc_rollout_plugin_prebuild -- never by a launch: the handle keeps what it loaded):
//
//   key = (L, N, q, trajectories per workgroup, lift variant, panel type, terminal refresh, diagnostics)
//   1. the process's table of loaded plug-ins (a second thread asking for a key that is being made waits for it; other keys do not),
//   2. the kernel cache on disk -- $KMPC_KERNEL_CACHE, <library directory>/kernel_cache (what __graft_entry__.build() pre-builds
//      travels with the tree), $XDG_CACHE_HOME/koopmpc, ~/.cache/koopmpc, $TMPDIR/koopmpc-<uid> -- file
//      rollout_L.._N.._q.._nw.._ks.._f64|f32[_term][_diag]_<hash>.so (ksm1: thin-plate RBF lift, ksm2: rbf.m's other kinds), the hash over the sources, the compiler flags and the compiler's --version, so
//      that a changed header or a new ROCm never meets a stale object,
//   3. hipcc on csrc/rollout_jit.hip (the sources ship next to the library) with the flags of the library's own build, 4-8 s per kernel,
//      under a file lock (the ranks of a node build an object once; the lock file stays), written under a temporary name and renamed,
//   then dlopen.  A plug-in is code this process runs, so the cache has a trust rule: a directory is used (read or written) only if
//   lstat shows a real directory -- not a symbolic link -- owned by this user and not writable by group or others, and an object is
//   loaded only if it is such a regular file.  Directories the library makes get mode 0700; the others are skipped and the status
//   text says why.  The plug-in has no undefined symbol of the library; its entry point gets the launch arguments and the workgroup
//   size.  A set that cannot be served (no compiler, no sources, no usable cache) leaves the handle on per-step launches and says why
//   (kmpc_rollout_plugin_status).
#include <dlfcn.h>
#include <fcntl.h>
#include <spawn.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "kernels.h"

extern char** environ;

namespace kmpc {

namespace {

struct Loaded {
  rollout_plugin_fn fn = nullptr;
  std::string path, how;
};
std::mutex g_mu;  // (guards the three tables; never held across a compile)
std::condition_variable g_cv;
typedef std::tuple<int, int, int, int, int, int, int, int> KeyTuple;
KeyTuple tuple_of(const RolloutPluginKey& k) { return std::make_tuple(k.L, k.N, k.q, k.nw, k.ks, k.io32, k.term, k.diag); }
std::map<KeyTuple, Loaded> g_loaded;
std::map<KeyTuple, std::string> g_failed;  // (a set that failed once is not compiled again and again)
std::set<KeyTuple> g_making;               // keys a thread of this process is looking up / compiling right now

const char* const kFlags[] = {"-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast", "-Wno-pass-failed", "-Wno-unused-function", "-shared"};
const char* const kSources[] = {"rollout_jit.hip", "rollout_kernel.hip", "step_body.h", "step_v2.h", "qp_rl.h", "kernels.h", "plant_device.h", "dare_device.h"};

std::string lib_dir() {
  Dl_info info{};
  if (!dladdr(reinterpret_cast<const void*>(&rollout_plugin_dims), &info) || !info.dli_fname) return "";
  std::string p(info.dli_fname);
  const size_t k = p.rfind('/');
  return k == std::string::npos ? std::string(".") : p.substr(0, k);
}
bool read_file(const std::string& path, std::string* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out->append(buf, n);
  fclose(f);
  return true;
}
std::string hipcc_path() {
  if (const char* e = getenv("KMPC_HIPCC")) { if (*e) return e; }
  if (access("/opt/rocm/bin/hipcc", X_OK) == 0) return "/opt/rocm/bin/hipcc";
  return "hipcc";
}

// the compiler as a child process (posix_spawn: the calling process, which may have initialised the GPU, is not replaced); its
// output (the last 64 KB) through a pipe into *out
bool run(const std::vector<std::string>& args, std::string* out, std::string* err) {
  std::vector<char*> argv;
  for (const auto& a : args) argv.push_back(const_cast<char*>(a.c_str()));
  argv.push_back(nullptr);
  int fd[2];
  if (pipe2(fd, O_CLOEXEC) != 0) { *err = std::string("pipe: ") + strerror(errno); return false; }
  posix_spawn_file_actions_t fa;
  posix_spawn_file_actions_init(&fa);
  posix_spawn_file_actions_adddup2(&fa, fd[1], 1);
  posix_spawn_file_actions_adddup2(&fa, fd[1], 2);
  posix_spawn_file_actions_addopen(&fa, 0, "/dev/null", O_RDONLY, 0);
  pid_t pid = 0;
  const int rc = posix_spawnp(&pid, argv[0], &fa, nullptr, argv.data(), environ);
  posix_spawn_file_actions_destroy(&fa);
  close(fd[1]);
  if (rc != 0) { close(fd[0]); *err = std::string("could not start ") + argv[0] + ": " + strerror(rc); return false; }
  char buf[4096];
  for (ssize_t n; (n = read(fd[0], buf, sizeof(buf))) != 0;) {
    if (n < 0) { if (errno == EINTR) continue; break; }
    out->append(buf, (size_t)n);
    if (out->size() > 65536) out->erase(0, out->size() - 65536);
  }
  close(fd[0]);
  int status = 0;
  while (waitpid(pid, &status, 0) < 0) {
    if (errno != EINTR) { *err = std::string("waitpid: ") + strerror(errno); return false; }
  }
  if (!WIFEXITED(status) || WEXITSTATUS(status) != 0) {
    *err = std::string(argv[0]) + " failed (" + (WIFEXITED(status) ? "exit code " + std::to_string(WEXITSTATUS(status)) : std::string("signal")) +
           "): ..." + (out->size() > 600 ? out->substr(out->size() - 600) : *out);
    return false;
  }
  return true;
}

// FNV-1a over the sources, the flags and the compiler's --version: the name of a cached object says what it was made of
// (once per process, source directory and compiler)
bool source_hash(const std::string& src_dir, const std::string& cc, unsigned long long* h, std::string* err) {
  static std::mutex mu;
  static std::map<std::string, unsigned long long> memo;
  std::lock_guard<std::mutex> lk(mu);
  auto it = memo.find(src_dir + '\n' + cc);
  if (it != memo.end()) { *h = it->second; return true; }
  unsigned long long x = 1469598103934665603ull;
  auto mix = [&](const char* p, size_t n) { for (size_t i = 0; i < n; ++i) { x ^= (unsigned char)p[i]; x *= 1099511628211ull; } };
  for (const char* s : kSources) {
    std::string body;
    if (!read_file(src_dir + "/" + s, &body)) { *err = "kernel source " + src_dir + "/" + s + " not found (the plug-in sources ship next to libkoopmpc.so)"; return false; }
    mix(body.data(), body.size());
  }
  for (const char* f : kFlags) mix(f, strlen(f));
  const int abi = KMPC_PLUGIN_ABI;
  mix(reinterpret_cast<const char*>(&abi), sizeof(abi));
  std::string ver;
  if (!run({cc, "--version"}, &ver, err)) return false;
  mix(ver.data(), ver.size());
  memo[src_dir + '\n' + cc] = x;
  *h = x;
  return true;
}

// the trust rule of the kernel cache: lstat shows a real directory (dir) / a regular file, owned by this user, not writable by group or
// others; *why says what failed
bool trusted(const std::string& p, bool dir, std::string* why) {
  struct stat st;
  if (lstat(p.c_str(), &st) != 0) { *why = strerror(errno); return false; }
  if (S_ISLNK(st.st_mode)) *why = "a symbolic link";
  else if (dir ? !S_ISDIR(st.st_mode) : !S_ISREG(st.st_mode)) *why = dir ? "not a directory" : "not a regular file";
  else if (st.st_uid != geteuid()) *why = "owned by uid " + std::to_string((long)st.st_uid);
  else if (st.st_mode & 022) { char b[64]; snprintf(b, sizeof(b), "writable by group or others (mode %03o)", (unsigned)(st.st_mode & 0777)); *why = b; }
  else return true;
  return false;
}
bool mkdir_p(const std::string& p) {
  if (p.empty()) return false;
  std::string cur;
  for (size_t i = 0; i <= p.size(); ++i) {
    if (i == p.size() || p[i] == '/') {
      if (!cur.empty() && cur != "/") { if (mkdir(cur.c_str(), 0700) != 0 && errno != EEXIST) return false; }
    }
    if (i < p.size()) cur.push_back(p[i]);
  }
  return true;
}
std::vector<std::string> cache_dirs() {
  std::vector<std::string> d;
  if (const char* e = getenv("KMPC_KERNEL_CACHE")) { if (*e) d.push_back(e); }
  const std::string ld = lib_dir();
  if (!ld.empty()) d.push_back(ld + "/kernel_cache");
  if (const char* x = getenv("XDG_CACHE_HOME")) { if (*x) d.push_back(std::string(x) + "/koopmpc"); }
  if (const char* h = getenv("HOME")) { if (*h) d.push_back(std::string(h) + "/.cache/koopmpc"); }
  const char* t = getenv("TMPDIR");
  d.push_back(std::string(t && *t ? t : "/tmp") + "/koopmpc-" + std::to_string((long)geteuid()));
  return d;
}

// measurement aid (KMPC_DEBUG only): extra compiler flags for the plug-ins, e.g. -DSOME_SWITCH=1 -- part of the object's hash, so that
// two settings are two objects (tools/dbg/ab_plugin.sh alternates them on one box; with KMPC_FORCE_PLUGIN the built-in sets run on plug-ins)
std::vector<std::string> extra_flags() {
  std::vector<std::string> out;
  const char* e = dbg_env("KMPC_PLUGIN_FLAGS");
  if (!e) return out;
  std::string cur;
  for (const char* p = e;; ++p) {
    if (*p == ' ' || *p == 0) { if (!cur.empty()) out.push_back(cur); cur.clear(); if (!*p) break; }
    else cur.push_back(*p);
  }
  return out;
}
std::string object_name(const RolloutPluginKey& k, unsigned long long h) {
  for (const auto& f : extra_flags())
    for (char ch : f) { h ^= (unsigned char)ch; h *= 1099511628211ull; }
  char buf[160];
  snprintf(buf, sizeof(buf), "rollout_L%d_N%d_q%d_nw%d_ks%s%d_%s%s%s_%016llx.so", k.L, k.N, k.q, k.nw, k.ks < 0 ? "m" : "", k.ks < 0 ? -k.ks : k.ks,
           k.io32 ? "f32" : "f64", k.term ? "_term" : "", k.diag ? "_diag" : "", h);
  return buf;
}

bool load_object(const std::string& path, Loaded* out, std::string* err) {
  void* lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!lib) { *err = std::string("dlopen ") + path + ": " + dlerror(); return false; }
  typedef int (*int_fn)(void);
  const int_fn abi = reinterpret_cast<int_fn>(dlsym(lib, "kmpc_rollout_plugin_abi"));
  const int_fn nb = reinterpret_cast<int_fn>(dlsym(lib, "kmpc_rollout_plugin_args_bytes"));
  const rollout_plugin_fn fn = reinterpret_cast<rollout_plugin_fn>(dlsym(lib, "kmpc_rollout_plugin_launch"));
  if (!abi || !nb || !fn || abi() != KMPC_PLUGIN_ABI || nb() != (int)sizeof(RolloutArgs<double>)) {
    dlclose(lib);
    *err = path + " is not a roll-out plug-in of this library version";
    return false;
  }
  out->fn = fn;
  out->path = path;
  return true;
}

// kernel cache, else hipcc (rollout_plugin_get calls it without g_mu: other keys are served meanwhile)
bool make_plugin(const RolloutPluginKey& k, Loaded* out, std::string* err) {
  const std::string ld = lib_dir();
  if (ld.empty()) { *err = "roll-out plug-in: cannot locate libkoopmpc.so (dladdr)"; return false; }
  const std::string src = ld + "/csrc", cc = hipcc_path();
  unsigned long long h = 0;
  if (!source_hash(src, cc, &h, err)) { *err = "roll-out plug-in: " + *err; return false; }
  const std::string name = object_name(k, h);
  std::string skipped, why;  // ("; skipped <path>: <why>" for what the trust rule turned down)
  std::vector<std::string> dirs;
  for (const auto& d : cache_dirs()) {
    struct stat st;
    if (lstat(d.c_str(), &st) != 0 || trusted(d, true, &why)) dirs.push_back(d);  // (a missing one is made when an object is written)
    else skipped += "; skipped " + d + ": " + why;
  }
  for (const auto& d : dirs) {
    const std::string p = d + "/" + name;
    if (access(p.c_str(), F_OK) != 0) continue;
    if (!trusted(p, false, &why)) skipped += "; skipped " + p + ": " + why;
    else if (load_object(p, out, err)) { out->how = "loaded from the kernel cache" + skipped; return true; }
  }
  std::string dir;
  for (const auto& d : dirs)
    if (mkdir_p(d) && trusted(d, true, &why) && access(d.c_str(), W_OK | X_OK) == 0) { dir = d; break; }
  if (dir.empty()) { *err = "roll-out plug-in: no usable kernel cache directory (set KMPC_KERNEL_CACHE)" + skipped; return false; }
  const std::string obj = dir + "/" + name, lock = obj + ".lock", tmp = obj + ".tmp." + std::to_string((long)getpid());
  // (the ranks of a node: one of them builds, the others find the object when they get the lock; the lock file is never removed, so
  //  that every process locks the same inode)
  const int lfd = open(lock.c_str(), O_CREAT | O_RDWR | O_NOFOLLOW | O_CLOEXEC, 0600);
  if (lfd < 0 || flock(lfd, LOCK_EX) != 0) {
    *err = "roll-out plug-in: lock " + lock + ": " + strerror(errno);
    if (lfd >= 0) close(lfd);
    return false;
  }
  const auto t0 = std::chrono::steady_clock::now();
  const bool build = access(obj.c_str(), F_OK) != 0;
  bool ok = true;
  if (build) {
    std::vector<std::string> args = {cc};
    for (const char* f : kFlags) args.push_back(f);
    args.push_back("-DKMPC_JIT_L=" + std::to_string(k.L));
    args.push_back("-DKMPC_JIT_N=" + std::to_string(k.N));
    args.push_back("-DKMPC_JIT_Q=" + std::to_string(k.q));
    args.push_back("-DKMPC_JIT_NW=" + std::to_string(k.nw));
    args.push_back("-DKMPC_JIT_KS=" + std::to_string(k.ks));
    args.push_back("-DKMPC_JIT_IO32=" + std::to_string(k.io32 ? 1 : 0));
    args.push_back("-DKMPC_JIT_TERM=" + std::to_string(k.term ? 1 : 0));
    args.push_back("-DKMPC_JIT_DIAG=" + std::to_string(k.diag ? 1 : 0));
    for (const auto& f : extra_flags()) args.push_back(f);
    for (const std::string& a : {"-I" + src, src + "/rollout_jit.hip", std::string("-o"), tmp}) args.push_back(a);
    std::string log;
    ok = run(args, &log, err);
    // (the object's mode does not depend on the umask: group- or world-writable objects are not loaded)
    if (ok && (chmod(tmp.c_str(), 0755) != 0 || rename(tmp.c_str(), obj.c_str()) != 0)) { *err = "rename " + tmp + ": " + strerror(errno); ok = false; }
    if (!ok) (void)unlink(tmp.c_str());
  }
  close(lfd);
  if (!ok) { *err = "roll-out plug-in " + name + ": " + *err; return false; }
  if (!trusted(obj, false, &why)) { *err = "roll-out plug-in: " + obj + ": " + why; return false; }
  if (!load_object(obj, out, err)) { *err = "roll-out plug-in: " + *err; return false; }
  char hb[96];
  snprintf(hb, sizeof(hb), build ? "compiled with hipcc in %.1f s" : "built by another process of this node (waited %.1f s)",
           std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  out->how = hb + skipped;
  return true;
}

}  // namespace

// Dimension sets a plug-in can be generated for: what rollout_kernel's two step bodies cover with one wave per trajectory --
//   y = C x with q <= 2 output rows: the register-state step (step_v2.h) for L + 2 <= 32, N <= 32; the LDS step (step_body.h) beyond,
//   y = psi (q = L): the 8 x 8-grid step of step_body.h,
// as far as sixteen / eight / four trajectories fit into a CU's LDS (the caller checks rollout_waves), n = 2 (the plants) and N <= 40.
// (q == L is read as y = psi: whether the handle's output kind agrees is the caller's question -- api.hip fused_kind_ok.)
static constexpr int kRolloutMaxHorizon = 40;
bool rollout_plugin_dims(int n, int L, int N, int q) {
  if (n != 2 || L < 2 || L > 64 || N < 2 || N > 64 || q < 1) return false;
  if (q != L && q > 2) return false;
  if ((long)(L + 1) * (L + 1) > 2048 || (long)N * N > 2048) return false;  // (beyond: four waves per trajectory, the per-step kernels)
  // The one-wave step solves horizons up to 40 in registers (step_body.h qp_regs).  Beyond, it runs the LDS solver, whose N x N tableau
  // needs a region that the roll-out's LDS layouts do not have (one region: none at all; two regions: sized without it where
  // tableau_saves_lds): at (44, 45, 2) the tableau ran over the next trajectory's region and the status words.  Per-step launches.
  if (N > kRolloutMaxHorizon) return false;
  return true;
}

rollout_plugin_fn rollout_plugin_get(const RolloutPluginKey& k, std::string* err) {
  const auto key = tuple_of(k);
  std::unique_lock<std::mutex> lk(g_mu);
  g_cv.wait(lk, [&] { return g_making.count(key) == 0; });
  auto it = g_loaded.find(key);
  if (it != g_loaded.end()) return it->second.fn;
  auto fi = g_failed.find(key);
  if (fi != g_failed.end()) { if (err) *err = fi->second; return nullptr; }
  g_making.insert(key);
  lk.unlock();
  Loaded L;
  std::string e;
  const bool ok = make_plugin(k, &L, &e);
  lk.lock();
  g_making.erase(key);
  if (ok) g_loaded[key] = L;
  else g_failed[key] = e;
  g_cv.notify_all();
  if (!ok && err) *err = e;
  return ok ? L.fn : nullptr;
}

std::string rollout_plugin_describe(const RolloutPluginKey& k) {
  const auto key = tuple_of(k);
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_loaded.find(key);
  if (it != g_loaded.end()) return "plug-in " + it->second.path + " (" + it->second.how + ")";
  auto fi = g_failed.find(key);
  if (fi != g_failed.end()) return "unavailable: " + fi->second;
  return "plug-in not loaded yet";
}

}  // namespace kmpc
