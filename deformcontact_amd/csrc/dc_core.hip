// dc_core.hip -- version + thread-local error string of libdeformcontact_hip.so.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "dc_common.h"

namespace dc {
static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int g_trace_on = 0;
static std::mutex g_trace_mu;
static std::map<std::string, int64_t> g_trace_counts;
// "(k_foo<A, B>)" as the launch macro sees it -> "k_foo<A, B>"
static std::string kernel_text(const char *name) {
    std::string n(name);
    while (!n.empty() && (n.front() == '(' || n.front() == ' ')) n.erase(n.begin());
    while (!n.empty() && (n.back() == ')' || n.back() == ' ')) n.pop_back();
    if (n.rfind("dc::", 0) == 0) n.erase(0, 4);
    return n;
}
static void trace_count_locked(const char *name) {
    if (g_trace_on & kTraceLog) ++g_trace_counts[kernel_text(name)];
}
void trace_kernel_slow(const char *name) {
    std::lock_guard<std::mutex> lock(g_trace_mu);
    trace_count_locked(name);
}

// ---- launch sites: the records DC_LAUNCH / DC_LAUNCH_SITE emit into the section "dc_sites" ----
extern "C" const Site __start_dc_sites[] __attribute__((visibility("hidden")));
extern "C" const Site __stop_dc_sites[] __attribute__((visibility("hidden")));
static size_t site_count() { return (size_t)(__stop_dc_sites - __start_dc_sites); }

// cumulative reached set (dc_launch_coverage), keyed on the record's address; g_site_test[i] is PYTEST_CURRENT_TEST at
// the first reach of site i ("" outside pytest), g_site_reached[i] the launches of site i while coverage was on (so that
// a caller can tell, from the difference around a call, exactly which sites that call launched).  dc_kernel_trace(1)
// does not touch them
static std::vector<int64_t> g_site_reached;
static std::vector<std::string> g_site_test;
void trace_site_slow(const Site *site, const char *name) {
    std::lock_guard<std::mutex> lock(g_trace_mu);
    trace_count_locked(name);
    if (!(g_trace_on & kTraceCoverage)) return;
    const size_t i = (size_t)(site - __start_dc_sites);
    if (i >= g_site_reached.size() || g_site_reached[i]++) return;
    const char *t = getenv("PYTEST_CURRENT_TEST");
    g_site_test[i] = t ? t : "";
}

static std::string collapse_ws(const std::string &s) {
    std::string out;
    for (char c : s) {
        const bool sp = c == ' ' || c == '\t' || c == '\n';
        if (!sp) out += c;
        else if (!out.empty() && out.back() != ' ') out += ' ';
    }
    while (!out.empty() && out.back() == ' ') out.pop_back();
    return out;
}

// A site's identity: "kernel text @ enclosing function" (kernel text normalised as in the launch log, whitespace
// collapsed).  Two launches of the same kernel expression in one function would share it: the later ones (in
// address order, which is source order) get " #2", " #3", ... so that neither can stand in for the other
static std::vector<std::string> site_ids() {
    std::vector<std::string> ids;
    std::map<std::string, int> seen;
    for (const Site *s = __start_dc_sites; s != __stop_dc_sites; ++s) {
        std::string id = collapse_ws(kernel_text(s->kernel)) + " @ " + collapse_ws(s->where);
        const int k = ++seen[id];
        if (k > 1) id += " #" + std::to_string(k);
        ids.push_back(id);
    }
    return ids;
}
static std::string base_name(const char *path) {
    const char *b = strrchr(path, '/');
    return b ? b + 1 : path;
}
static int64_t copy_out(const std::string &out, char *buf, int64_t cap) {
    if (buf && cap > 0) {
        const size_t n = out.size() < (size_t)cap - 1 ? out.size() : (size_t)cap - 1;
        memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return (int64_t)out.size() + 1;
}
}  // namespace dc

// Launch sites.  dc_launch_sites_dump: every site the library was built with, one "source file \t identity\n" line
// each (host data only: works without a GPU).  dc_launch_coverage(1) starts / (0) stops adding the sites that launch
// to a cumulative reached set (never cleared; independent of dc_kernel_trace); dc_launch_reached_dump writes
// "identity \t PYTEST_CURRENT_TEST at the first reach \t launches while coverage was on\n" lines.  Both dumps: NUL-terminated, truncated to cap, return
// the bytes the full text needs.
extern "C" int64_t dc_launch_sites_dump(char *buf, int64_t cap) {
    const std::vector<std::string> ids = dc::site_ids();
    std::string out;
    for (size_t i = 0; i < ids.size(); ++i)
        out += dc::base_name(dc::__start_dc_sites[i].file) + "\t" + ids[i] + "\n";
    return dc::copy_out(out, buf, cap);
}
extern "C" void dc_launch_coverage(int on) {
    std::lock_guard<std::mutex> lock(dc::g_trace_mu);
    if (on && dc::g_site_reached.empty()) {
        dc::g_site_reached.assign(dc::site_count(), 0);
        dc::g_site_test.assign(dc::site_count(), std::string());
    }
    dc::g_trace_on = (dc::g_trace_on & ~dc::kTraceCoverage) | (on ? dc::kTraceCoverage : 0);
}
extern "C" int64_t dc_launch_reached_dump(char *buf, int64_t cap) {
    const std::vector<std::string> ids = dc::site_ids();
    std::lock_guard<std::mutex> lock(dc::g_trace_mu);
    std::string out;
    for (size_t i = 0; i < dc::g_site_reached.size(); ++i)
        if (dc::g_site_reached[i]) out += ids[i] + "\t" + dc::g_site_test[i] + "\t" + std::to_string(dc::g_site_reached[i]) + "\n";
    return dc::copy_out(out, buf, cap);
}

// Launch log: dc_kernel_trace(1) clears it and starts counting every kernel launch of the library by kernel name (as
// written at the launch site, e.g. "k_fwd_h2w<true, false>"; template PARAMETERS of the host function stay
// symbolic, e.g. "k_hop_chain_gcn<STEPS>"), dc_kernel_trace(0) stops; dc_kernel_trace_dump writes "name count\n"
// lines (NUL-terminated, truncated to cap) and returns the bytes the full text needs.
extern "C" void dc_kernel_trace(int on) {
    std::lock_guard<std::mutex> lock(dc::g_trace_mu);
    if (on) dc::g_trace_counts.clear();
    dc::g_trace_on = (dc::g_trace_on & ~dc::kTraceLog) | (on ? dc::kTraceLog : 0);
}
extern "C" int64_t dc_kernel_trace_dump(char *buf, int64_t cap) {
    std::lock_guard<std::mutex> lock(dc::g_trace_mu);
    std::string out;
    for (const auto &kv : dc::g_trace_counts) out += kv.first + " " + std::to_string(kv.second) + "\n";
    return dc::copy_out(out, buf, cap);
}

extern "C" int dc_version(void) { return 200; }   // 0.2.0
extern "C" const char *dc_last_error(void) { return dc::g_err; }

extern "C" int64_t dc_stream_capture_id(dc_stream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    if (hipStreamGetCaptureInfo((hipStream_t)stream, &st, &id) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return st == hipStreamCaptureStatusActive ? (int64_t)id : 0;
}
