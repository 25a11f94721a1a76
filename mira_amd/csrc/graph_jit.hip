// The run-time compiler behind mira_graph_specialize (graph_jit.hpp writes the source): hiprtc, loaded with dlopen at the
// first use, and the code objects of earlier processes on disk (mira_graph_set_cache_dir).
#include "ctx.h"
#include "graph_jit.hpp"
#ifndef MIRA_CPU_EMU
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "jit_headers.inc"
namespace graphjit {
Rtc &rtc() {
    static Rtc loaded = [] {
        Rtc r;
        for (const char *name : {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (r.lib) break;
        }
        if (!r.lib) { r.error = "libhiprtc.so not found: graphs stay interpreted"; return r; }
        auto sym = [&](const char *n) { void *p = dlsym(r.lib, n); if (!p) r.error = std::string("libhiprtc.so lacks ") + n; return p; };
        r.create = reinterpret_cast<decltype(r.create)>(sym("hiprtcCreateProgram"));
        r.compile = reinterpret_cast<decltype(r.compile)>(sym("hiprtcCompileProgram"));
        r.log_size = reinterpret_cast<decltype(r.log_size)>(sym("hiprtcGetProgramLogSize"));
        r.log = reinterpret_cast<decltype(r.log)>(sym("hiprtcGetProgramLog"));
        r.code_size = reinterpret_cast<decltype(r.code_size)>(sym("hiprtcGetCodeSize"));
        r.code = reinterpret_cast<decltype(r.code)>(sym("hiprtcGetCode"));
        r.destroy = reinterpret_cast<decltype(r.destroy)>(sym("hiprtcDestroyProgram"));
        return r;
    }();
    return loaded;
}
// A specialised kernel keeps the in-place multiplier (field29.cuh: F29_COLUMN_SERIAL): hiprtc compiles its straight-line program of
// several hundred products four times slower around the column-serial form (10.8 -> 46 s for the main gate's kernels, LAB_NOTES),
// for 3 % of evaluation throughput.  Compiled once per circuit, but in front of its first fold.
static const char *const JIT_OPTIONS[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-DF29_COLUMN_SERIAL=0"};
static constexpr int JIT_OPTION_COUNT = (int)(sizeof(JIT_OPTIONS) / sizeof(JIT_OPTIONS[0]));
std::vector<char> compile(const std::string &src, std::string &err) {
    Rtc &r = rtc();
    std::vector<char> out;
    if (!r.error.empty()) { err = r.error; return out; }
    void *prog = nullptr;
    // the kernel headers travel inside the library: `#include "field29.cuh"` (and its own includes) resolve to these texts
    if (r.create(&prog, src.c_str(), "mira_jit.hip", JIT_HDR_COUNT, const_cast<const char **>(JIT_HDR_TEXT), const_cast<const char **>(JIT_HDR_NAME)) != 0) {
        err = "hiprtcCreateProgram failed";
        return out;
    }
    const int rc = r.compile(prog, JIT_OPTION_COUNT, const_cast<const char **>(JIT_OPTIONS));
    if (rc != 0) {
        size_t n = 0;
        (void)r.log_size(prog, &n);
        std::string log(n, 0);
        if (n > 1) (void)r.log(prog, &log[0]);
        err = "hiprtcCompileProgram failed (" + std::to_string(rc) + "): " + log.substr(0, 2000);
        (void)r.destroy(&prog);
        return out;
    }
    size_t n = 0;
    if (r.code_size(prog, &n) == 0 && n) { out.resize(n); if (r.code(prog, out.data()) != 0) out.clear(); }
    if (out.empty()) err = "hiprtcGetCode failed";
    (void)r.destroy(&prog);
    return out;
}

// ---- code objects on disk (mira_graph_set_cache_dir) --------------------------------------------------------------
// A file per kernel: magic | key of the build environment | source length | source | code length | hash of the code | code.
// The file name is a hash of source and environment; a hit must match both byte for byte and the code must hash to what the
// header says, so a colliding, stale or damaged file (other kernel headers, another ROCm, another GPU architecture, a
// truncated write) is a miss, never a wrong kernel.  The hash guards against damage, not against an adversary: a code object
// is executed on the GPU as it is, so the directory must belong to the user and be writable by nobody else -- checked when it
// is set and again for every file that is taken.
static std::string g_cache_dir;
static uint64_t fnv1a(const void *p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}
static bool read_file(const std::string &path, std::vector<char> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    struct stat sb;
    if (fstat(fileno(f), &sb) != 0 || sb.st_uid != geteuid() || (sb.st_mode & (S_IWGRP | S_IWOTH))) { fclose(f); return false; }   // somebody else's file, or one others may write
    out.clear();
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    const bool ok = !ferror(f);
    fclose(f);
    return ok;
}
// everything besides the source text that decides the code object: the embedded headers, the compiler options, the GPU
// architecture the process runs on, the HIP runtime and the hiprtc that compiles
static const std::string &environment_key() {
    static const std::string key = [] {
        Rtc &r = rtc();
        uint64_t h = 0xcbf29ce484222325ull;
        for (int i = 0; i < JIT_HDR_COUNT; i++) {
            h = fnv1a(JIT_HDR_TEXT[i], strlen(JIT_HDR_TEXT[i]), h);
            h = fnv1a(JIT_HDR_NAME[i], strlen(JIT_HDR_NAME[i]), h);
        }
        std::string opts;
        for (const char *o : JIT_OPTIONS) { opts += o; opts += ' '; }
        int major = 0, minor = 0, runtime = 0;
        if (r.lib) {
            auto version = reinterpret_cast<int (*)(int *, int *)>(dlsym(r.lib, "hiprtcVersion"));
            if (version) (void)version(&major, &minor);
        }
        (void)hipRuntimeGetVersion(&runtime);
        hipDeviceProp_t prop;
        std::string arch = "unknown";
        if (hipGetDeviceProperties(&prop, g.device) == hipSuccess) arch = prop.gcnArchName;
        char buf[96];
        snprintf(buf, sizeof buf, "%016llx", (unsigned long long)h);
        return "mira-jit-2 arch " + arch + " hip " + std::to_string(runtime) + " hiprtc " + std::to_string(major) + "." + std::to_string(minor) + " headers " + buf + " options " + opts;
    }();
    return key;
}
static std::string cache_path(const std::string &src) {
    const std::string &env = environment_key();
    const uint64_t a = fnv1a(src.data(), src.size()), b = fnv1a(env.data(), env.size(), a ^ 0x9e3779b97f4a7c15ull);
    char name[64];
    snprintf(name, sizeof name, "/mira_jit_%016llx%016llx.bin", (unsigned long long)a, (unsigned long long)b);
    return g_cache_dir + name;
}
static constexpr char CACHE_MAGIC[8] = {'M', 'I', 'R', 'A', 'J', 'I', 'T', '2'};
static void code_hash(const std::vector<char> &code, uint64_t out[2]) {
    out[0] = fnv1a(code.data(), code.size());
    out[1] = fnv1a(code.data(), code.size(), 0x84222325cbf29ce4ull ^ code.size());
}
std::vector<char> cache_load(const std::string &src) {
    std::vector<char> file, code;
    if (g_cache_dir.empty() || !read_file(cache_path(src), file)) return code;
    const std::string &env = environment_key();
    size_t pos = 0;
    auto take = [&](const void *want, size_t n) { const bool ok = pos + n <= file.size() && memcmp(file.data() + pos, want, n) == 0; pos += n; return ok; };
    auto take_len = [&](uint64_t &v) { if (pos + 8 > file.size()) return false; memcpy(&v, file.data() + pos, 8); pos += 8; return true; };
    uint64_t n_env = 0, n_src = 0, n_code = 0, want[2] = {0, 0}, have[2];
    if (!take(CACHE_MAGIC, 8) || !take_len(n_env) || n_env != env.size() || !take(env.data(), env.size())) return code;
    if (!take_len(n_src) || n_src != src.size() || !take(src.data(), src.size())) return code;
    if (!take_len(n_code) || !take_len(want[0]) || !take_len(want[1]) || n_code == 0 || pos + n_code != file.size()) return code;
    code.assign(file.begin() + (long)pos, file.end());
    code_hash(code, have);
    if (have[0] != want[0] || have[1] != want[1]) code.clear();
    return code;
}
void cache_store(const std::string &src, const std::vector<char> &code) {   // best effort: a failure costs the next process a compilation
    if (g_cache_dir.empty() || code.empty()) return;
    const std::string path = cache_path(src), tmp = path + ".tmp" + std::to_string((unsigned long long)getpid());
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0600);
    FILE *f = fd >= 0 ? fdopen(fd, "wb") : nullptr;
    if (!f) { if (fd >= 0) close(fd); return; }
    const std::string &env = environment_key();
    uint64_t hash[2];
    code_hash(code, hash);
    const uint64_t n_env = env.size(), n_src = src.size(), n_code = code.size();
    bool ok = fwrite(CACHE_MAGIC, 1, 8, f) == 8 && fwrite(&n_env, 8, 1, f) == 1 && fwrite(env.data(), 1, env.size(), f) == env.size();
    ok = ok && fwrite(&n_src, 8, 1, f) == 1 && fwrite(src.data(), 1, src.size(), f) == src.size();
    ok = ok && fwrite(&n_code, 8, 1, f) == 1 && fwrite(hash, 8, 2, f) == 2 && fwrite(code.data(), 1, code.size(), f) == code.size();
    ok = (fclose(f) == 0) && ok;
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) (void)remove(tmp.c_str());   // rename: readers see a whole file or none
}
}   // namespace graphjit

// Directory for the code objects of specialised kernels, or null / "" for none (the default): a later process -- or this
// one after mira_graph_free -- that specialises the same graph loads the kernel instead of compiling it.
int graph_set_cache_dir(const char *dir) {
    std::string d = dir ? dir : "";
    while (d.size() > 1 && d.back() == '/') d.pop_back();
    if (!d.empty()) {
        // code objects found there are executed on the GPU: the directory must be the user's own, writable by nobody else
        struct stat sb;
        if (stat(d.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode)) { set_error(d + " is not a directory"); return MIRA_E_IO; }
        if (sb.st_uid != geteuid() || (sb.st_mode & (S_IWGRP | S_IWOTH))) {
            set_error(d + " must belong to the calling user and be writable by nobody else (mode 0700 or 0755): kernels found there are executed");
            return MIRA_E_BAD_ARG;
        }
    }
    graphjit::g_cache_dir = d;
    return MIRA_OK;
}
// source text -> code object size, through the library's own hiprtc path and embedded headers; needs no device
int graph_jit_compile_check(const char *src, size_t *code_size_out) {
    if (!src) { set_error("null source"); return MIRA_E_BAD_ARG; }
    if (!graphjit::rtc().error.empty()) { set_error(graphjit::rtc().error); return MIRA_E_JIT_UNAVAILABLE; }
    std::string err;
    const std::vector<char> code = graphjit::compile(src, err);
    if (code.empty()) { set_error(err); return MIRA_E_JIT_FAILED; }
    if (code_size_out) *code_size_out = code.size();
    return MIRA_OK;
}
#else
int graph_set_cache_dir(const char *) { return MIRA_OK; }
int graph_jit_compile_check(const char *, size_t *) {
    set_error("the host emulation has no run-time compiler");
    return MIRA_E_JIT_UNAVAILABLE;
}
#endif
