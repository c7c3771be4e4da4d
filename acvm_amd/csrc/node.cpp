// node.cpp -- the node-level driver behind the C ABI (include/acvm_amd.h acvm_node_*): ONE call solves a global batch of witness
// instances of one circuit on every GPU of the node. It replaces the loop a caller of the reference runs once per instance
// (acvm_js/src/execute.rs:60-119: ACVM::new, solve, finalize / error string, witness extraction) and does what SURVEY 8e describes:
//   * the global batch is split contiguously over the devices (device d owns instances [d * per, (d + 1) * per)), no exchange step;
//   * per device one host thread drives one batch handle (one levelised plan, one witness table) through its shard in tiles;
//   * the inputs of tile k + 1 travel host -> pinned staging -> device beside the solve of tile k (a second thread per device fills
//     the two staging buffers and issues hipMemcpyAsync on a copy stream);
//   * instances that leave the generic path are re-solved by the exact kernels in a side table on a stream of their own, beside the
//     level schedule of the NEXT tile (batch.cpp, asynchronous exact path): a few diverging inputs per tile do not stall the tile;
//   * per instance the caller gets the result record, the kept witnesses (normally the circuit's return values) and the 32-byte
//     digest of the whole witness map, in global instance order.
// acvm_node_solve_device is the same driver for callers whose data lives on the GPUs: per lane the inputs are read from, and kept witnesses,
// outcome columns, digests and the selection written into, device memory of that lane (run_lane_device_body; checks and tile views:
// node_io_plan.cpp). No staging, no producer thread; the exact path still runs beside the next tile and writes its rows on the device.
// Both forms answer Brillig foreign calls through the node's handler, per tile, behind the tile's solve and in front of its export (foreign_rounds:
// execute.rs:109-113; the host-only decisions: node_foreign_plan.cpp). Without a handler the rows leave in RequiresForeignCall.
#include "batch.hpp"
#include "circuit.hpp"
#include "node_foreign_plan.hpp"
#include "node_io_plan.hpp"
#include "record_plan.hpp"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <mutex>
#include <pthread.h>
#include <sched.h>
#include <thread>
#include <unistd.h>

namespace {

struct DeviceLane {
    int device = 0;
    acvm_batch_t *batch = nullptr;
    bool async = false;
    uint8_t *pinned[2] = {nullptr, nullptr};
    uint8_t *d_in[2] = {nullptr, nullptr};
    hipStream_t copy = nullptr, out = nullptr;  // uploads of the producer thread; downloads of the kept witnesses
    hipEvent_t ev_h2d[2] = {nullptr, nullptr};
    hipEvent_t ev_imported[2] = {nullptr, nullptr};  // the import kernel has read staging slot k: the next upload into it may start
    hipEvent_t ev_exported[2] = {nullptr, nullptr}, ev_arrived[2] = {nullptr, nullptr};  // kept witnesses: export kernel done / copy in pinned memory
    // kept witnesses leave the device beside the NEXT tile's solve: export kernel + D2H into pinned memory are enqueued behind a solve and
    // harvested after the following one
    uint32_t *d_keep = nullptr;
    uint8_t *d_exp[2] = {nullptr, nullptr}, *h_exp[2] = {nullptr, nullptr};
    // statistics of the last solve
    double device_ms = 0, h2d_wait_ms = 0, export_ms = 0, total_ms = 0;
    uint32_t tiles = 0, exact_instances = 0;
    uint64_t not_solved = 0;
    uint64_t io_h2d = 0, io_d2h = 0;  // bytes the device form copied for this lane, cumulative (acvm_debug_node_io_bytes)
    std::string error;
    int rc = 0;
    // the foreign-call handler's round trips (foreign_rounds): device scratch for a site's inputs and for an answer uploaded from host memory (both
    // grow-only), host staging for a host-space handler, the statistics of the last node call
    uint32_t index = 0;
    uint8_t *d_fc = nullptr, *d_fc_ans = nullptr;
    uint64_t fc_cap = 0, fc_ans_cap = 0;
    std::vector<uint8_t> h_fc;
    acvm_node_foreign_stats_t fc{};
    // host placement: the CPUs local to the device (sysfs), empty = unknown / not pinned
    int numa_node = -1;
    std::vector<uint32_t> cpus;
};

// "0-15,32-47" (sysfs cpulist format) -> CPU numbers; anything malformed ends the list where it stands
std::vector<uint32_t> parse_cpulist(const std::string &text) {
    std::vector<uint32_t> out;
    size_t i = 0;
    auto number = [&](uint32_t &v) {
        if (i >= text.size() || text[i] < '0' || text[i] > '9') return false;
        uint64_t x = 0;
        while (i < text.size() && text[i] >= '0' && text[i] <= '9' && x < (1u << 20)) x = x * 10 + (uint64_t)(text[i++] - '0');
        v = (uint32_t)x;
        return x < (1u << 20);
    };
    while (i < text.size()) {
        uint32_t a, b;
        if (!number(a)) break;
        b = a;
        if (i < text.size() && text[i] == '-') { i++; if (!number(b) || b < a) break; }
        for (uint32_t c = a; c <= b && out.size() < 4096; c++) out.push_back(c);
        if (i < text.size() && text[i] == ',') i++;
        else break;
    }
    return out;
}
// NUMA node and local CPUs of a PCI device from sysfs (<root>/<bus id>/numa_node, local_cpulist); false if the files are not there
bool device_locality(const std::string &pci_root, const std::string &bus_id, int *numa_node, std::vector<uint32_t> *cpus) {
    std::string id = bus_id;
    for (char &ch : id) ch = (char)tolower((unsigned char)ch);
    std::ifstream fn(pci_root + "/" + id + "/numa_node"), fc(pci_root + "/" + id + "/local_cpulist");
    if (!fn || !fc) return false;
    int node = -1;
    fn >> node;
    std::string list;
    std::getline(fc, list);
    *numa_node = node;
    *cpus = parse_cpulist(list);
    return true;
}
// the calling thread onto the given CPUs (and with it every thread it creates from now on); silently not when the set is empty or refused
// (only CPUs the process may use at all: the device's local list is intersected with the thread's current mask -- a container's cpuset, a
// caller's taskset; an empty intersection leaves the thread where it is)
void pin_thread(const std::vector<uint32_t> &cpus) {
    if (cpus.empty()) return;
    cpu_set_t allowed, set;
    CPU_ZERO(&allowed);
    const bool have_allowed = pthread_getaffinity_np(pthread_self(), sizeof allowed, &allowed) == 0;
    CPU_ZERO(&set);
    int n = 0;
    for (uint32_t c : cpus)
        if (c < CPU_SETSIZE && (!have_allowed || CPU_ISSET(c, &allowed))) { CPU_SET(c, &set); n++; }
    if (n) (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);
}
// threads that are joined when the scope ends, whichever way it ends
struct Joiner {
    std::vector<std::thread> t;
    ~Joiner() {
        for (auto &x : t)
            if (x.joinable()) x.join();
    }
};

// a node call is running (acvm_node_set_foreign_call_handler refuses meanwhile)
struct RunningCall {
    std::atomic<int> &count;
    explicit RunningCall(acvm_node *n);
    ~RunningCall() { count.fetch_sub(1); }
};

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

struct acvm_node {
    std::vector<DeviceLane> lanes;
    std::vector<uint32_t> ids, keep;
    uint32_t tile = 0, flags = 0;
    uint64_t last_n = 0;
    double last_total_ms = 0;
    std::shared_ptr<const Plan> plan;  // the one plan every lane's handle shares
    uint32_t plans_built = 0;          // how often acvm_node_new levelised the circuit (0: the circuit's cache already held the plan; never more than 1)
    double create_ms = 0, plan_ms = 0;
    // the foreign-call handler (acvm_node_set_foreign_call_handler): read by the lanes' threads during a node call, changed only between calls
    bool has_solver = false, has_handler = false;
    acvm_node_foreign_handler_t handler{};
    std::atomic<int> running{0};
    ~acvm_node() {
        for (DeviceLane &l : lanes) {
            hipSetDevice(l.device);
            if (l.batch) acvm_batch_free(l.batch);
            for (int k = 0; k < 2; k++) {
                if (l.pinned[k]) hipHostFree(l.pinned[k]);
                if (l.d_in[k]) hipFree(l.d_in[k]);
                for (hipEvent_t e : {l.ev_h2d[k], l.ev_imported[k], l.ev_exported[k], l.ev_arrived[k]})
                    if (e) hipEventDestroy(e);
                if (l.d_exp[k]) hipFree(l.d_exp[k]);
                if (l.h_exp[k]) hipHostFree(l.h_exp[k]);
            }
            if (l.d_keep) hipFree(l.d_keep);
            if (l.d_fc) hipFree(l.d_fc);
            if (l.d_fc_ans) hipFree(l.d_fc_ans);
            if (l.copy) hipStreamDestroy(l.copy);
            if (l.out) hipStreamDestroy(l.out);
        }
    }
};

namespace {

RunningCall::RunningCall(acvm_node *n) : count(n->running) { count.fetch_add(1); }

// instances per handle when the caller leaves the choice to the library: the largest power of two (at most 2^17, the measured optimum of
// the 10k-gate circuit, NOTEBOOK.md section 7) that every listed device has room for. Per device: 90 % of its free memory, less the lookup
// tables the circuit would still build there, divided by the number of handles the device is listed for; a handle needs its tables, class
// scratch and first side table (batch_device_bytes) plus this driver's staging and export buffers.
uint32_t auto_tile(const Plan &p, const PlanOpts &opts, const std::vector<uint32_t> &ids, const std::vector<uint32_t> &keep, const std::vector<int> &devices) {
    const bool pedersen_level = !p.cls_offset[CLS_PEDERSEN].empty();
    const bool window_table = pedersen_level && p.tune.pedersen_window_bits != 0;
    double budget = 1e30;
    for (int d : devices) {
        size_t free_b = 0, total_b = 0;
        if (hipSetDevice(d) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) { set_err(ACVM_E_DEVICE, "hipMemGetInfo failed"); return 0; }
        const double tables = (double)device_tables_missing_bytes(p.needs_grumpkin, pedersen_level, window_table, p.needs_ecdsa);
        const double copies = (double)std::count(devices.begin(), devices.end(), d);
        budget = std::min(budget, (0.9 * (double)free_b - tables) / copies);
    }
    const double io_per_instance = 2.0 * 32.0 * (double)ids.size() * 2.0 /* pinned + device staging are separate pools; count the device one twice for slack */ +
                                   2.0 * 32.0 * (double)keep.size();
    uint32_t t = 1u << 17;
    while (t > 64 && (double)batch_device_bytes(p, opts, t, true) + io_per_instance * t > budget) t >>= 1;
    if ((double)batch_device_bytes(p, opts, t, true) + io_per_instance * t > budget) { set_err(ACVM_E_DEVICE, "not enough free device memory for a tile of 64 instances of this circuit"); return 0; }
    return t;
}

// rows [first, first + n) of the caller's inputs into a pinned buffer (a partial tile fills and uploads its own rows only: batch_set_live_count)
// (a tile of the 10k-gate circuit is 64 MB: one core copies that in ~10 ms, which would be exposed in front of the first tile; four do it in ~3)
void fill_staging(uint8_t *dst, const uint8_t *values, size_t row, uint64_t first, uint32_t n) {
    if (row == 0) return;
    const uint8_t *src = values + first * row;
    const size_t bytes = (size_t)n * row;
    constexpr size_t PIECE = 8u << 20;
    if (bytes <= 2 * PIECE) memcpy(dst, src, bytes);
    else {
        const size_t part = (bytes / 4 + 63) / 64 * 64;
        Joiner helpers;  // (a thread that cannot be created throws: the ones that run are joined before the exception leaves)
        for (int q = 0; q < 3; q++)
            helpers.t.emplace_back([=] { const size_t at = (size_t)(q + 1) * part; if (at < bytes) memcpy(dst + at, src + at, std::min(part, bytes - at)); });
        memcpy(dst, src, std::min(part, bytes));
    }
}

// an outcome of the exact path of the tile that started at global instance `base` (n_valid instances of it are the caller's)
uint64_t patch_outcome(const ExactOutcome &o, uint64_t base, uint32_t n_valid, uint32_t n_keep, acvm_result_t *results, uint8_t *kept, uint8_t *kept_assigned,
                       uint8_t *digests) {
    uint64_t not_solved = 0;
    for (size_t t = 0; t < o.instance.size(); t++) {
        const uint32_t j = o.instance[t];
        if (j >= n_valid) continue;
        const uint64_t g = base + j;
        not_solved += o.results[t].status != ACVM_STATUS_SOLVED;
        if (results) results[g] = o.results[t];
        if (kept && n_keep && !o.kept_values.empty()) memcpy(kept + g * n_keep * 32, &o.kept_values[t * (size_t)n_keep * 32], (size_t)n_keep * 32);
        if (kept_assigned && n_keep && !o.kept_assigned.empty()) memcpy(kept_assigned + g * n_keep, &o.kept_assigned[t * (size_t)n_keep], n_keep);
        if (digests && !o.digests.empty()) memcpy(digests + g * 32, &o.digests[t * 32], 32);
    }
    return not_solved;
}

// a grow-only device buffer of the lane; false: no memory (the old buffer is gone, the capacity says so)
bool grow_device(uint8_t **d, uint64_t *cap, uint64_t need) {
    const uint64_t want = node_foreign_grow(*cap, need);
    if (!want) return true;
    if (*d) hipFree(*d);
    *d = nullptr;
    *cap = 0;
    if (hipMalloc((void **)d, want) != hipSuccess) { (void)hipGetLastError(); *d = nullptr; return false; }
    *cap = want;
    return true;
}

// The foreign-call loop of one tile, behind its acvm_batch_solve and in front of its export (include/acvm_amd.h acvm_node_set_foreign_call_handler;
// the reference's caller: acvm_js/src/execute.rs:109-113 per instance): per round every site the handle lists is handed to the handler with its
// inputs in the lane's scratch, the answer goes through acvm_batch_resolve_foreign_calls_device_rows, and the tile is solved again. The host-only
// decisions are node_foreign_plan.cpp's. A failure sets L.rc / L.error; the callers' L.rc paths leave the handle reusable.
void foreign_rounds(acvm_node *node, DeviceLane &L, uint32_t tile_index, uint64_t row_base) {
    if (!node->has_handler || L.rc) return;
    const acvm_node_foreign_handler_t &H = node->handler;
    auto fail = [&](int rc, const std::string &what) { if (!L.rc) { L.rc = rc; L.error = what + ": " + acvm_last_error(); } };
    auto fail_text = [&](int rc, const std::string &text) { if (!L.rc) { L.rc = rc; L.error = text; } };
    const uint32_t max_rounds = node_foreign_max_rounds(H.max_rounds), in_size = buffer_element_size(H.in_encoding);
    const bool host = H.space == ACVM_SPACE_HOST;
    uint64_t h2d0 = 0, d2h0 = 0, own_h2d = 0, own_d2h = 0;
    acvm_debug_foreign_call_stats(L.batch, &h2d0, &d2h0, nullptr, nullptr, nullptr);
    std::vector<acvm_foreign_call_site_t> sites;
    std::vector<uint64_t> declined;  // sites the handler declined for this tile
    auto key_of = [](const acvm_foreign_call_site_t &s) { return ((uint64_t)s.opcode_index << 32) | s.brillig_index; };
    auto list_sites = [&]() -> bool {
        int ns = acvm_batch_foreign_call_sites(L.batch, nullptr, 0);
        if (ns > 0) {
            sites.resize((size_t)ns);
            ns = acvm_batch_foreign_call_sites(L.batch, sites.data(), (uint32_t)ns);
        }
        if (ns < 0) { fail(ns, "foreign-call sites"); return false; }
        sites.resize(std::min(sites.size(), (size_t)ns));
        return true;
    };
    auto name_of = [&](const acvm_foreign_call_site_t &s, uint32_t round) {
        char fn[65] = {0};
        memcpy(fn, s.function, 64);
        return "lane " + std::to_string(L.index) + ", tile " + std::to_string(tile_index) + ", round " + std::to_string(round) + ", site (opcode " +
               std::to_string(s.opcode_index) + ", brillig index " + std::to_string(s.brillig_index) + ", '" + fn + "')";
    };
    for (uint32_t round = 0; !L.rc; round++) {
        if (!list_sites()) break;
        sites.erase(std::remove_if(sites.begin(), sites.end(), [&](const acvm_foreign_call_site_t &s) { return std::find(declined.begin(), declined.end(), key_of(s)) != declined.end(); }),
                    sites.end());
        if (sites.empty()) break;
        if (round >= max_rounds) {  // the cap: what still waits is reported, and exported as RequiresForeignCall
            for (const acvm_foreign_call_site_t &s : sites) L.fc.rows_left_waiting += s.n_waiting;
            break;
        }
        L.fc.rounds++;
        uint64_t resumed = 0;
        const std::vector<acvm_foreign_call_site_t> asked = sites;  // (list_sites below reuses `sites`)
        for (const acvm_foreign_call_site_t &s : asked) {
            const uint32_t n_rows = s.n_waiting;
            // ---- the inputs of the site's list into the lane's scratch: the sizing call, then the columns
            acvm_foreign_call_inputs_desc_t d{};
            d.opcode_index = s.opcode_index;
            d.brillig_index = s.brillig_index;
            d.n_rows = n_rows;
            d.encoding = H.in_encoding;
            d.layout = H.in_layout;
            uint32_t longest = 0;
            if (int rc = acvm_batch_foreign_call_inputs_device(L.batch, &d, &longest)) { fail(rc, "foreign-call inputs of " + name_of(s, round)); break; }
            NodeForeignInputs sc;
            if (!node_foreign_inputs_scratch(n_rows, s.n_inputs, longest, in_size, &sc) || !grow_device(&L.d_fc, &L.fc_cap, sc.bytes)) {
                fail_text(ACVM_E_NOMEM, "no device memory for the foreign-call inputs of " + name_of(s, round));
                break;
            }
            d.n_columns = longest;
            d.d_instances = (uint32_t *)(L.d_fc + sc.o_rows);
            d.d_lens = (uint32_t *)(L.d_fc + sc.o_lens);
            d.d_values = longest ? L.d_fc + sc.o_values : nullptr;
            d.d_mask = longest ? L.d_fc + sc.o_mask : nullptr;
            if (int rc = acvm_batch_foreign_call_inputs_device(L.batch, &d, nullptr)) { fail(rc, "foreign-call inputs of " + name_of(s, round)); break; }
            const uint8_t *base = L.d_fc;
            if (host) {  // (the inputs call returned after the batch's stream was waited for)
                L.h_fc.resize((size_t)sc.bytes);
                hipError_t e = hipSuccess;
                const std::pair<uint64_t, uint64_t> parts[4] = {{sc.o_rows, sc.rows_bytes}, {sc.o_lens, sc.lens_bytes}, {sc.o_values, sc.values_bytes}, {sc.o_mask, sc.mask_bytes}};
                for (const auto &part : parts)
                    if (e == hipSuccess && part.second) e = hipMemcpyAsync(L.h_fc.data() + part.first, L.d_fc + part.first, (size_t)part.second, hipMemcpyDeviceToHost, L.copy);
                if (e == hipSuccess) e = hipStreamSynchronize(L.copy);
                if (e != hipSuccess) { fail_text(ACVM_E_DEVICE, std::string("download of the foreign-call inputs: ") + hipGetErrorString(e)); break; }
                own_d2h += sc.rows_bytes + sc.lens_bytes + sc.values_bytes + sc.mask_bytes;
                base = L.h_fc.data();
            }
            // ---- the handler
            acvm_node_foreign_round_t in{};
            in.lane = L.index;
            in.device = L.device;
            in.tile = tile_index;
            in.round = round;
            in.site = s;
            in.n_rows = n_rows;
            in.max_values = longest;
            in.row_base = row_base;
            in.rows = (const uint32_t *)(base + sc.o_rows);
            in.lens = (const uint32_t *)(base + sc.o_lens);
            in.values = base + sc.o_values;
            in.mask = base + sc.o_mask;
            acvm_node_foreign_answer_t out{};
            const double t0 = now_ms();
            const int returned = H.fn(H.user, &in, &out);
            L.fc.handler_ms += now_ms() - t0;
            L.fc.handler_calls++;
            int abort_rc = 0;
            const NodeForeignVerdict verdict = node_foreign_verdict(returned, &abort_rc);
            if (verdict == NODE_FOREIGN_ABORT) { fail_text(abort_rc, "the foreign-call handler returned " + std::to_string(returned) + " for " + name_of(s, round)); break; }
            if (hipSetDevice(L.device) != hipSuccess) { fail_text(ACVM_E_DEVICE, "hipSetDevice behind the foreign-call handler"); break; }  // (whatever the handler made current)
            if (verdict == NODE_FOREIGN_DECLINED) {
                declined.push_back(key_of(s));
                L.fc.rows_declined += n_rows;
                continue;
            }
            // ---- the answer: from host memory it goes up into the lane's scratch first; then the one resolve path
            acvm_foreign_call_answers_rows_desc_t a{};
            a.opcode_index = s.opcode_index;
            a.brillig_index = s.brillig_index;
            a.n_rows = n_rows;
            a.n_values = out.n_values;
            a.is_array = out.is_array;
            a.lens = out.lens;
            a.encoding = out.encoding;
            a.layout = out.layout;
            a.n_columns = out.n_columns;
            a.stride = out.stride;
            a.d_values = out.values;
            a.d_lens = out.row_lens;
            a.d_answered = out.answered;
            if (host) {
                NodeForeignAnswer as;
                std::string text;
                if (int rc = node_foreign_answer_scratch(&out, n_rows, &as, &text)) { fail_text(rc, "the answer for " + name_of(s, round) + ": " + text); break; }
                if (!grow_device(&L.d_fc_ans, &L.fc_ans_cap, as.bytes)) { fail_text(ACVM_E_NOMEM, "no device memory for the answer for " + name_of(s, round)); break; }
                hipError_t e = hipSuccess;
                if (as.values_bytes) e = hipMemcpyAsync(L.d_fc_ans + as.o_values, out.values, (size_t)as.values_bytes, hipMemcpyHostToDevice, L.copy);
                if (e == hipSuccess && as.lens_bytes) e = hipMemcpyAsync(L.d_fc_ans + as.o_lens, out.row_lens, (size_t)as.lens_bytes, hipMemcpyHostToDevice, L.copy);
                if (e == hipSuccess && as.answered_bytes) e = hipMemcpyAsync(L.d_fc_ans + as.o_answered, out.answered, (size_t)as.answered_bytes, hipMemcpyHostToDevice, L.copy);
                if (e == hipSuccess) e = hipStreamSynchronize(L.copy);  // (the handler's memory is read until here)
                if (e != hipSuccess) { fail_text(ACVM_E_DEVICE, std::string("upload of the foreign-call answer: ") + hipGetErrorString(e)); break; }
                own_h2d += as.values_bytes + as.lens_bytes + as.answered_bytes;
                a.d_values = as.values_bytes ? L.d_fc_ans + as.o_values : nullptr;
                a.d_lens = out.row_lens ? (const uint32_t *)(L.d_fc_ans + as.o_lens) : nullptr;
                a.d_answered = out.answered ? L.d_fc_ans + as.o_answered : nullptr;
            }
            if (int rc = acvm_batch_resolve_foreign_calls_device_rows(L.batch, &a)) { fail(rc, "the answer for " + name_of(s, round)); break; }
            // the rows the answer resumed: the site's n_resolved (host only)
            if (!list_sites()) break;
            uint32_t now_resolved = 0;
            for (const acvm_foreign_call_site_t &q : sites)
                if (key_of(q) == key_of(s)) now_resolved = q.n_resolved;
            const uint32_t answered = now_resolved > s.n_resolved ? now_resolved - s.n_resolved : 0u;
            L.fc.rows_answered += answered;
            L.fc.rows_declined += n_rows - std::min(n_rows, answered);
            resumed += answered;
        }
        if (L.rc || !resumed) break;  // nobody resumes: no further solve
        const int rc = acvm_batch_solve(L.batch);
        if (rc < 0) { fail(rc, "solve behind the foreign-call round " + std::to_string(round) + " of tile " + std::to_string(tile_index)); break; }
        acvm_stats_t st;
        acvm_batch_stats(L.batch, &st);
        L.device_ms += st.solve_device_ms;
    }
    uint64_t h2d1 = h2d0, d2h1 = d2h0;
    acvm_debug_foreign_call_stats(L.batch, &h2d1, &d2h1, nullptr, nullptr, nullptr);
    L.fc.h2d_bytes += h2d1 - h2d0 + own_h2d;
    L.fc.d2h_bytes += d2h1 - d2h0 + own_d2h;
    L.io_h2d += h2d1 - h2d0 + own_h2d;
    L.io_d2h += d2h1 - d2h0 + own_d2h;
}

// rec: null, or the record descriptor of acvm_node_solve_records (checked by the caller): `values` are then host records of rec->pitch bytes, a
// tile stages and uploads m * pitch bytes and is imported through the record plan; everything else is the same.
void run_lane_body(acvm_node *node, DeviceLane &L, uint64_t first, uint64_t last, const uint8_t *values, const acvm_record_desc_t *rec, acvm_result_t *results, uint8_t *kept,
                   uint8_t *kept_assigned, uint8_t *digests) {
    const double t_begin = now_ms();
    L.rc = 0;
    L.error.clear();
    L.device_ms = L.h2d_wait_ms = L.export_ms = 0;
    L.tiles = L.exact_instances = 0;
    L.not_solved = 0;
    L.fc = acvm_node_foreign_stats_t{};
    auto fail = [&](int rc, const std::string &what) { if (!L.rc) { L.rc = rc; L.error = what + ": " + acvm_last_error(); } };
    if (hipSetDevice(L.device) != hipSuccess) { fail(ACVM_E_DEVICE, "hipSetDevice"); return; }
    const uint32_t tile = node->tile, n_keep = (uint32_t)node->keep.size();
    const size_t row = rec ? (rec->n_fields ? (size_t)rec->pitch : 0) : node->ids.size() * 32;
    const uint64_t n = last - first;
    const uint32_t n_tiles = (uint32_t)((n + tile - 1) / tile);
    if (!n_tiles) return;
    // ---- producer: host rows -> pinned staging -> device, one tile ahead of the solver. Every failure of it reaches the solver (producer_rc):
    // a solver that waited for a tile that never comes would hang, one that went on after a failed copy would solve stale inputs.
    std::mutex mu;
    std::condition_variable cv;
    uint32_t staged = 0, consumed = 0;  // tiles whose H2D was issued / whose import was enqueued (the staging slot is handed back through ev_imported)
    bool abort = false;
    int producer_rc = 0;
    std::string producer_err;
    std::thread producer([&] {
        auto give_up_rc = [&](int rc, const std::string &what) {
            {
                std::lock_guard<std::mutex> lk(mu);
                producer_rc = rc;
                producer_err = what;
            }
            cv.notify_all();
        };
        auto give_up = [&](const char *what, hipError_t e) { give_up_rc(ACVM_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); };
        try {  // nothing unwinds out of a thread (std::terminate) nor through the ABI: an allocation failure ends the lane with ACVM_E_NOMEM
        if (hipError_t e = hipSetDevice(L.device); e != hipSuccess) { give_up("hipSetDevice (upload thread)", e); return; }  // HIP's current device is per thread
        for (uint32_t k = 0; k < n_tiles; k++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return abort || k < consumed + 2; });
                if (abort) return;
            }
            const uint64_t base = first + (uint64_t)k * tile;
            const uint32_t m = (uint32_t)std::min<uint64_t>(tile, last - base);
            const int slot = (int)(k & 1);
            // the pinned half of the slot is free once its previous upload has been read by the copy engine (ev_h2d, waited for by the solver
            // before it enqueued that tile's import), the device half once that import kernel has run (ev_imported)
            if (k >= 2)
                if (hipError_t e = hipStreamWaitEvent(L.copy, L.ev_imported[slot], 0); e != hipSuccess) { give_up("hipStreamWaitEvent", e); return; }
            fill_staging(L.pinned[slot], values, row, base, m);
            if (row)
                if (hipError_t e = hipMemcpyAsync(L.d_in[slot], L.pinned[slot], (size_t)m * row, hipMemcpyHostToDevice, L.copy); e != hipSuccess) { give_up("hipMemcpyAsync (upload)", e); return; }
            if (hipError_t e = hipEventRecord(L.ev_h2d[slot], L.copy); e != hipSuccess) { give_up("hipEventRecord", e); return; }
            {
                std::lock_guard<std::mutex> lk(mu);
                staged = k + 1;
            }
            cv.notify_all();
        }
        } catch (const std::bad_alloc &) {
            give_up_rc(ACVM_E_NOMEM, "out of host memory in the upload thread");
        } catch (const std::exception &e) {
            give_up_rc(ACVM_E_INVALID, std::string("upload thread: ") + e.what());
        }
    });
    auto stop_producer = [&] {
        {
            std::lock_guard<std::mutex> lk(mu);
            abort = true;
        }
        cv.notify_all();
        producer.join();
    };
    try {  // (an exception of the solver side -- std::bad_alloc of its bookkeeping vectors -- must not skip the join of the producer below)
    // ---- solver
    uint64_t prev_base = 0;
    uint32_t prev_valid = 0;
    bool in_flight = false;  // kept witnesses of a tile on their way to pinned memory
    int fl_slot = 0;
    uint64_t fl_base = 0;
    uint32_t fl_n = 0;
    std::vector<uint32_t> fl_flagged;
    auto harvest = [&]() -> bool {  // the kept witnesses of the tile in flight: wait for their copy (it ran beside the solve that followed), scatter
        if (!in_flight) return true;
        in_flight = false;
        if (hipEventSynchronize(L.ev_arrived[fl_slot]) != hipSuccess) { fail(ACVM_E_DEVICE, "hipEventSynchronize (kept witnesses)"); return false; }
        memcpy(kept + fl_base * n_keep * 32, L.h_exp[fl_slot], (size_t)fl_n * n_keep * 32);
        std::vector<uint8_t> flagged(fl_n, 0);
        for (uint32_t j : fl_flagged)
            if (j < fl_n) flagged[j] = 1;
        for (uint32_t k2 = 0; k2 < n_keep; k2++) {  // the level kernels' assigned set is the planner's
            const bool produced = batch_generic_assigned(L.batch, node->keep[k2]);
            for (uint32_t j = 0; j < fl_n; j++) {
                if (flagged[j]) continue;
                if (kept_assigned) kept_assigned[(fl_base + j) * n_keep + k2] = produced;
                if (!produced) memset(kept + ((fl_base + j) * n_keep + k2) * 32, 0, 32);
            }
        }
        return true;
    };
    for (uint32_t k = 0; k < n_tiles && !L.rc; k++) {
        const uint64_t base = first + (uint64_t)k * tile;
        const uint32_t m = (uint32_t)std::min<uint64_t>(tile, last - base);
        const int slot = (int)(k & 1);
        const double t0 = now_ms();
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return staged > k || producer_rc != 0; });
            if (producer_rc) { L.rc = producer_rc; L.error = "upload of tile " + std::to_string(k) + ": " + producer_err; break; }
        }
        if (hipEventSynchronize(L.ev_h2d[slot]) != hipSuccess) { fail(ACVM_E_DEVICE, "hipEventSynchronize"); break; }
        L.h2d_wait_ms += now_ms() - t0;
        if (int rc = batch_set_live_count(L.batch, m)) { fail(rc, "live count"); break; }  // a partial last tile: the lanes behind it are dead
        // the import is enqueued, not waited for: it runs behind the export kernel of the previous tile and in front of this tile's levels
        if (int rc = rec ? batch_import_records_async(L.batch, rec, L.d_in[slot], L.ev_imported[slot]) : batch_import_async(L.batch, L.d_in[slot], L.ev_imported[slot])) {
            fail(rc, "set_initial_witness");
            break;
        }
        {   // the producer may prepare the tile after next (its upload waits for ev_imported on the copy stream)
            std::lock_guard<std::mutex> lk(mu);
            consumed = k + 1;
        }
        cv.notify_all();
        const int rc = acvm_batch_solve(L.batch);  // asynchronous handles: collects the exact job of tile k - 1 on the way
        if (rc < 0) { fail(rc, "solve"); break; }
        acvm_stats_t st;
        acvm_batch_stats(L.batch, &st);
        L.device_ms += st.solve_device_ms;
        L.exact_instances += st.n_slow_instances;
        L.tiles++;
        foreign_rounds(node, L, k, node_foreign_row_base(false, first, k, tile));  // (no handler: nothing)
        if (L.rc) break;
        const double t1 = now_ms();
        // the kept witnesses of the PREVIOUS tile: their copy ran on the download stream beside this solve
        if (!harvest()) break;
        if (k > 0) {
            ExactOutcome o;
            batch_take_outcome(L.batch, &o);
            if (!o.instance.empty()) L.not_solved += patch_outcome(o, prev_base, prev_valid, n_keep, results, kept, kept_assigned, digests);
        }
        const bool pending = batch_exact_pending(L.batch);
        const std::vector<uint32_t> &exact_ids = *batch_exact_instances(L.batch);
        L.not_solved += batch_exact_unsolved(L.batch, m);  // (a synchronous exact path: its lanes are final)
        // instances of a SYNCHRONOUS exact path have their values (and assigned sets) where only the batch knows: such a tile exports in one
        // synchronous step; every other tile enqueues its kept witnesses and goes on
        const bool overlap = kept && n_keep && (exact_ids.empty() || pending);
        if (int rc2 = batch_export_tile(L.batch, m, node->keep.data(), overlap ? 0u : n_keep, results ? results + base : nullptr,
                                        kept && !overlap ? kept + base * n_keep * 32 : nullptr, kept_assigned && !overlap ? kept_assigned + base * n_keep : nullptr,
                                        digests ? digests + base * 32 : nullptr)) {
            fail(rc2, "export");
            break;
        }
        if (overlap) {
            if (int rc3 = batch_enqueue_kept(L.batch, m, L.d_keep, n_keep, L.d_exp[slot], L.h_exp[slot], L.out, L.ev_exported[slot], L.ev_arrived[slot])) { fail(rc3, "export of the kept witnesses"); break; }
            in_flight = true;
            fl_slot = slot;
            fl_base = base;
            fl_n = m;
            fl_flagged.assign(exact_ids.begin(), exact_ids.end());  // (arrive with the exact job's outcome)
        }
        L.export_ms += now_ms() - t1;
        prev_base = base;
        prev_valid = m;
    }
    if (!L.rc) harvest();
    if (!L.rc) {  // the exact job of the last tile
        ExactOutcome o;
        if (int rc = batch_finish_pending(L.batch, &o)) fail(rc, "exact path");
        else L.not_solved += patch_outcome(o, prev_base, prev_valid, n_keep, results, kept, kept_assigned, digests);
    }
    } catch (const std::bad_alloc &) {
        if (!L.rc) { L.rc = ACVM_E_NOMEM; L.error = "out of host memory in the lane's solver thread"; }
    } catch (const std::exception &e) {
        if (!L.rc) { L.rc = ACVM_E_INVALID; L.error = std::string("lane: ") + e.what(); }
    }
    stop_producer();
    hipStreamSynchronize(L.copy);
    hipStreamSynchronize(L.out);
    if (L.rc) {  // leave the handle reusable
        ExactOutcome o;
        batch_finish_pending(L.batch, &o);
        acvm_device_synchronize();  // (an import enqueued for a tile that was never solved)
    }
    L.total_ms = now_ms() - t_begin;
}

// The lane body of the device form (acvm_node_solve_device): the lane's rows are where the caller's producer left them and its outcomes stay
// where the caller's consumer reads them, so there is no producer thread, no pinned staging and nothing to harvest. Per tile: live count,
// import of the tile's view (node_io_plan.cpp: the address rule), solve, then kept witnesses, outcome columns and digests of the instances the
// level kernels solved are ENQUEUED into the caller's buffers -- nothing in the loop waits for the pending exact job, which runs beside the
// next tile as in run_lane_body; its rows are written on the device when its outcome is collected (batch_set_exact_sink).
void run_lane_device_body(acvm_node *node, DeviceLane &L, const NodeLaneIo &lane, acvm_node_lane_io_t *io) {
    const double t_begin = now_ms();
    L.rc = 0;
    L.error.clear();
    L.device_ms = L.h2d_wait_ms = L.export_ms = 0;
    L.tiles = L.exact_instances = 0;
    L.not_solved = 0;
    L.fc = acvm_node_foreign_stats_t{};
    io->n_selected = io->not_solved = 0;
    auto fail = [&](int rc, const std::string &what) { if (!L.rc) { L.rc = rc; L.error = what + ": " + acvm_last_error(); } };
    auto fail_hip = [&](const char *what, hipError_t e) { if (!L.rc) { L.rc = ACVM_E_DEVICE; L.error = std::string(what) + ": " + hipGetErrorString(e); } };
    L.total_ms = 0;
    if (!lane.n_tiles) return;
    if (hipError_t e = hipSetDevice(L.device); e != hipSuccess) { fail_hip("hipSetDevice", e); return; }
    const NodeIoShape shape{(uint32_t)node->ids.size(), (uint32_t)node->keep.size(), node->tile};
    const uint32_t n = (uint32_t)lane.io.n;
    // the selection runs over the lane's status column: a scratch one when the caller wants none
    NodeLaneIo view = lane;
    uint8_t *d_scratch_status = nullptr;
    uint32_t *d_scan = nullptr;
    const size_t scan_words = select_scratch_words(n) + 1;  // (the count behind the scan's scratch)
    if (!view.io.d_status) {
        if (hipError_t e = hipMalloc((void **)&d_scratch_status, n); e != hipSuccess) { fail_hip("hipMalloc (status column)", e); return; }
        view.io.d_status = d_scratch_status;
    }
    if (hipError_t e = hipMalloc((void **)&d_scan, scan_words * 4); e != hipSuccess) { fail_hip("hipMalloc (selection)", e); hipFree(d_scratch_status); return; }
    const uint64_t list_copies = acvm_debug_import_list_copies(L.batch);
    auto sink_of = [&](const NodeTileIo &t) {
        TileSink k;
        k.n = t.m;
        k.encoding = view.io.kept_encoding;
        k.layout = view.io.kept_layout;
        k.d_keep = L.d_keep;
        k.n_keep = shape.n_keep;
        k.stride = t.kept_stride;
        k.d_kept = t.d_kept;
        k.d_kept_assigned = t.d_kept_assigned;
        k.d_status = t.d_status;
        k.d_err = t.d_err;
        k.d_opcode_index = t.d_opcode_index;
        k.d_digests = t.d_digests32;
        k.h2d = &L.io_h2d;
        return k;
    };
    auto count_outcome = [&](const ExactOutcome &o, uint32_t n_valid) {
        for (size_t t = 0; t < o.instance.size(); t++) L.not_solved += o.instance[t] < n_valid && o.results[t].status != ACVM_STATUS_SOLVED;
    };
    try {
    uint32_t prev_valid = 0;
    for (uint32_t k = 0; k < lane.n_tiles && !L.rc; k++) {
        NodeTileIo t;
        std::string text;
        if (int rc = node_io_tile(shape, view, k, &t, &text)) { L.rc = rc; L.error = text; break; }
        if (int rc = batch_set_live_count(L.batch, t.m)) { fail(rc, "live count"); break; }
        if (int rc = batch_import_desc_async(L.batch, &t.in, t.d_values)) { fail(rc, "import"); break; }
        const int rc = acvm_batch_solve(L.batch);  // asynchronous handles: collects the exact job of tile k - 1 on the way, into that tile's sink
        if (rc < 0) { fail(rc, "solve"); break; }
        acvm_stats_t st;
        acvm_batch_stats(L.batch, &st);
        L.device_ms += st.solve_device_ms;
        L.exact_instances += st.n_slow_instances;
        L.tiles++;
        foreign_rounds(node, L, k, node_foreign_row_base(true, 0, k, node->tile));  // (no handler: nothing)
        if (L.rc) break;
        const double t1 = now_ms();
        if (k > 0) {
            ExactOutcome o;
            batch_take_outcome(L.batch, &o);
            count_outcome(o, prev_valid);
        }
        L.not_solved += batch_exact_unsolved(L.batch, t.m);  // (a synchronous exact path: its lanes are final)
        const TileSink sink = sink_of(t);
        if (int rc2 = batch_enqueue_tile_outcomes(L.batch, &sink)) { fail(rc2, "outcomes"); break; }
        batch_set_exact_sink(L.batch, &sink);
        L.export_ms += now_ms() - t1;
        prev_valid = t.m;
    }
    if (!L.rc) {  // the exact job of the last tile
        ExactOutcome o;
        if (int rc = batch_finish_pending(L.batch, &o)) fail(rc, "exact path");
        else count_outcome(o, prev_valid);
    }
    if (!L.rc)
        if (int rc = batch_stream_synchronize(L.batch)) fail(rc, "synchronize");
    if (!L.rc) {  // one selection over the whole lane, behind the last outcome
        uint32_t count = 0;
        launch_select(L.out, view.io.d_status, 0, n, view.io.select_mask, d_scan, view.io.d_selected, d_scan + scan_words - 1);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&count, d_scan + scan_words - 1, 4, hipMemcpyDeviceToHost, L.out);
        if (e == hipSuccess) e = hipStreamSynchronize(L.out);
        if (e != hipSuccess) fail_hip("selection", e);
        L.io_d2h += 4;
        io->n_selected = count;
    }
    } catch (const std::bad_alloc &) {
        if (!L.rc) { L.rc = ACVM_E_NOMEM; L.error = "out of host memory in the lane's solver thread"; }
    } catch (const std::exception &e) {
        if (!L.rc) { L.rc = ACVM_E_INVALID; L.error = std::string("lane: ") + e.what(); }
    }
    if (L.rc) {  // leave the handle reusable (the sink of a job in flight is still the caller's memory: it is written or dropped here)
        ExactOutcome o;
        batch_finish_pending(L.batch, &o);
        acvm_device_synchronize();
    }
    L.io_h2d += (acvm_debug_import_list_copies(L.batch) - list_copies) * (uint64_t)shape.n_in * 4;  // (the column list, when it changed)
    hipFree(d_scratch_status);
    hipFree(d_scan);
    io->not_solved = L.not_solved;
    L.total_ms = now_ms() - t_begin;
}

void run_lane_device(acvm_node *node, DeviceLane &L, const NodeLaneIo &lane, acvm_node_lane_io_t *io) {
    try {
        pin_thread(L.cpus);
        run_lane_device_body(node, L, lane, io);
    } catch (const std::bad_alloc &) {
        if (!L.rc) { L.rc = ACVM_E_NOMEM; L.error = "out of host memory"; }
    } catch (const std::exception &e) {
        if (!L.rc) { L.rc = ACVM_E_INVALID; L.error = e.what(); }
    } catch (...) {
        if (!L.rc) { L.rc = ACVM_E_INVALID; L.error = "unknown exception"; }
    }
}

// a lane's thread: pinned to the CPUs of its device's NUMA node (its upload thread and the staging helpers inherit the mask), and closed
// against exceptions: std::terminate is not an error code
void run_lane(acvm_node *node, DeviceLane &L, uint64_t first, uint64_t last, const uint8_t *values, const acvm_record_desc_t *rec, acvm_result_t *results, uint8_t *kept,
              uint8_t *kept_assigned, uint8_t *digests) {
    try {
        pin_thread(L.cpus);
        run_lane_body(node, L, first, last, values, rec, results, kept, kept_assigned, digests);
    } catch (const std::bad_alloc &) {
        if (!L.rc) { L.rc = ACVM_E_NOMEM; L.error = "out of host memory"; }
    } catch (const std::exception &e) {
        if (!L.rc) { L.rc = ACVM_E_INVALID; L.error = e.what(); }
    } catch (...) {
        if (!L.rc) { L.rc = ACVM_E_INVALID; L.error = "unknown exception"; }
    }
}

}  // namespace

extern "C" {

acvm_node_t *acvm_node_new(const acvm_circuit_t *c, const acvm_bb_solver_t *solver, const uint32_t *initial_ids, uint32_t n_initial, const uint32_t *keep_ids,
                           uint32_t n_keep, const acvm_node_opts_t *opts) try {
    if (!c || (n_initial && !initial_ids) || (n_keep && !keep_ids)) { set_err(ACVM_E_INVALID, "null argument"); return nullptr; }
    const int visible = acvm_device_count();
    if (visible < 1) { set_err(ACVM_E_DEVICE, "no HIP device visible; the library has no CPU fallback"); return nullptr; }
    auto node = std::make_unique<acvm_node>();
    node->ids.assign(initial_ids, initial_ids + n_initial);
    node->keep.assign(keep_ids, keep_ids + n_keep);
    // a kept witness beyond the circuit is simply never assigned (WitnessMap::get -> None): on the device it travels as 0xFFFFFFFF, "no row"
    for (uint32_t &w : node->keep)
        if (w >= acvm_circuit_num_witnesses(c)) w = 0xFFFFFFFFu;
    node->flags = opts ? opts->batch_flags : 0;
    node->has_solver = solver != nullptr;
    std::vector<int> devices;
    // n_devices == 0 selects every visible device and `devices` is not read (it holds n_devices entries: none)
    const bool listed = opts && opts->n_devices && opts->devices;
    const uint32_t n_dev = opts && opts->n_devices ? opts->n_devices : (uint32_t)visible;
    if (n_dev > 16) { set_err(ACVM_E_INVALID, "at most 16 handles per node (acvm_node_stats_t)"); return nullptr; }
    for (uint32_t i = 0; i < n_dev; i++) {
        const int d = listed ? opts->devices[i] : (int)i;
        if (d < 0 || d >= visible) { set_err(ACVM_E_INVALID, "device index " + std::to_string(d) + " out of range (" + std::to_string(visible) + " visible)"); return nullptr; }
        devices.push_back(d);
    }
    // The circuit is levelised ONCE per node (the reference's callers build one opcode list per circuit for any number of executions,
    // acvm_js/src/execute.rs:60-119): the plan is immutable and shared -- auto_tile sizes the handles by it and every lane's
    // acvm_batch_new_ex finds it in the circuit's plan cache (batch.cpp plan_for) instead of planning again (until round 5: 1 + N times).
    const double t_create = now_ms();
    const uint64_t built_before = acvm_circuit_plans_built(c);
    {
        PlanOpts po;  // exactly what acvm_batch_new_ex derives from the same arguments
        po.host_blackbox = solver != nullptr;
        po.fold_digest = (node->flags & (ACVM_BATCH_FOLD_DIGEST | ACVM_BATCH_REUSE_SLOTS)) != 0;
        po.reuse_slots = (node->flags & ACVM_BATCH_REUSE_SLOTS) != 0;
        po.keep = node->keep;
        node->plan = plan_for(c, node->ids.data(), n_initial, po);
        if (!node->plan->unsupported.empty()) { set_err(ACVM_E_UNSUPPORTED, node->plan->unsupported); return nullptr; }
        node->plan_ms = node->plan->plan_ms;
        node->tile = opts && opts->tile_instances ? opts->tile_instances : auto_tile(*node->plan, po, node->ids, node->keep, devices);
    }
    if (!node->tile) return nullptr;
    node->lanes.resize(devices.size());
    const size_t row = (size_t)n_initial * 32;
    // one handle per device, created side by side (each allocates tens of GB and levelises the circuit)
    std::vector<std::thread> th;
    for (size_t i = 0; i < devices.size(); i++) {
        node->lanes[i].device = devices[i];
        node->lanes[i].index = (uint32_t)i;
        th.emplace_back([&, i] {
            DeviceLane &L = node->lanes[i];
            try {  // (nothing leaves a thread: std::terminate is not an error code)
            auto fail = [&](int rc, const std::string &what) { L.rc = rc; L.error = what + ": " + acvm_last_error(); };
            if (hipSetDevice(L.device) != hipSuccess) { L.rc = ACVM_E_DEVICE; L.error = "hipSetDevice failed"; return; }
            {   // where the device hangs: its NUMA node and the CPUs next to it (pinned staging is allocated and filled from there)
                char bus[32] = {0};
                if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, L.device) == hipSuccess) device_locality("/sys/bus/pci/devices", bus, &L.numa_node, &L.cpus);
                else (void)hipGetLastError();
                pin_thread(L.cpus);  // (this thread allocates the lane's pinned buffers: first touch on the device's node)
            }
            L.batch = acvm_batch_new_ex(c, solver, node->tile, node->ids.data(), n_initial, node->flags, node->keep.data(), n_keep);
            if (!L.batch) { fail(ACVM_E_DEVICE, "acvm_batch_new_ex"); return; }
            const int a = batch_enable_async_exact(L.batch, node->keep.data(), n_keep, true);
            if (a < 0) { fail(a, "async exact path"); return; }
            L.async = a == 1;
            const size_t bytes = std::max<size_t>((size_t)node->tile * row, 16);
            bool ok = hipStreamCreateWithFlags(&L.copy, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&L.out, hipStreamNonBlocking) == hipSuccess;
            for (int k = 0; k < 2 && ok; k++)
                ok = hipHostMalloc((void **)&L.pinned[k], bytes, hipHostMallocDefault) == hipSuccess && hipMalloc((void **)&L.d_in[k], bytes) == hipSuccess &&
                     hipEventCreateWithFlags(&L.ev_h2d[k], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&L.ev_imported[k], hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&L.ev_exported[k], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&L.ev_arrived[k], hipEventDisableTiming) == hipSuccess;
            if (ok && n_keep) {
                const size_t eb = (size_t)node->tile * n_keep * 32;
                ok = hipMalloc((void **)&L.d_keep, (size_t)n_keep * 4) == hipSuccess &&
                     hipMemcpy(L.d_keep, node->keep.data(), (size_t)n_keep * 4, hipMemcpyHostToDevice) == hipSuccess;
                for (int k = 0; k < 2 && ok; k++)
                    ok = hipMalloc((void **)&L.d_exp[k], eb) == hipSuccess && hipHostMalloc((void **)&L.h_exp[k], eb, hipHostMallocDefault) == hipSuccess;
            }
            if (!ok) { L.rc = ACVM_E_DEVICE; L.error = "staging buffers: allocation failed"; }
            } catch (const std::bad_alloc &) {
                if (!L.rc) { L.rc = ACVM_E_NOMEM; L.error = "out of host memory"; }
            } catch (const std::exception &e) {
                if (!L.rc) { L.rc = ACVM_E_INVALID; L.error = e.what(); }
            } catch (...) {
                if (!L.rc) { L.rc = ACVM_E_INVALID; L.error = "unknown exception"; }
            }
        });
    }
    for (auto &t : th) t.join();
    for (DeviceLane &L : node->lanes)
        if (L.rc) { set_err(L.rc, "device " + std::to_string(L.device) + ": " + L.error); return nullptr; }
    node->plans_built = (uint32_t)(acvm_circuit_plans_built(c) - built_before);
    node->create_ms = now_ms() - t_create;
    return node.release();
} ABI_CATCH_PTR

void acvm_node_free(acvm_node_t *n) { delete n; }

uint32_t acvm_node_tile_instances(const acvm_node_t *n) { return n ? n->tile : 0; }
uint32_t acvm_node_num_devices(const acvm_node_t *n) { return n ? (uint32_t)n->lanes.size() : 0; }

namespace {
// the body of acvm_node_solve and acvm_node_solve_records (rec: null, or the checked record descriptor that `values` are read by)
long long node_solve_host(acvm_node_t *n, uint64_t n_instances, const uint8_t *values_be32, const acvm_record_desc_t *rec, acvm_result_t *results, uint8_t *kept_be32,
                          uint8_t *kept_assigned, uint8_t *digests32) {
    RunningCall running(n);
    const double t0 = now_ms();
    const size_t D = n->lanes.size();
    // contiguous split, multiples of 64 instances per device except the last
    std::vector<uint64_t> bound(D + 1, 0);
    const uint64_t per = ((n_instances + D - 1) / D + 63) / 64 * 64;
    for (size_t d = 0; d <= D; d++) bound[d] = std::min<uint64_t>(n_instances, per * d);
    std::vector<std::thread> th;
    for (size_t d = 0; d < D; d++)
        th.emplace_back(run_lane, n, std::ref(n->lanes[d]), bound[d], bound[d + 1], values_be32, rec, results, kept_be32, kept_assigned, digests32);
    for (auto &t : th) t.join();
    n->last_n = n_instances;
    n->last_total_ms = now_ms() - t0;
    for (DeviceLane &L : n->lanes)
        if (L.rc) return set_err(L.rc, "device " + std::to_string(L.device) + ": " + L.error);
    long long not_solved = 0;
    for (DeviceLane &L : n->lanes) not_solved += (long long)L.not_solved;
    return not_solved;
}
}  // namespace

long long acvm_node_solve(acvm_node_t *n, uint64_t n_instances, const uint8_t *values_be32, acvm_result_t *results, uint8_t *kept_be32, uint8_t *kept_assigned,
                          uint8_t *digests32) try {
    if (!n || (n_instances && !n->ids.empty() && !values_be32)) return set_err(ACVM_E_INVALID, "null argument");
    return node_solve_host(n, n_instances, values_be32, nullptr, results, kept_be32, kept_assigned, digests32);
} ABI_CATCH

// The inputs as host records: the descriptor is checked once, here, before any lane starts (record_plan.cpp; rows and planes are the lanes' own
// and do not enter the checks), then every lane's tiles go through batch_import_records_async.
long long acvm_node_solve_records(acvm_node_t *n, uint64_t n_instances, const acvm_record_desc_t *in, const void *records, acvm_result_t *results, uint8_t *kept_be32,
                                  uint8_t *kept_assigned, uint8_t *digests32) try {
    if (!n) return set_err(ACVM_E_INVALID, "null argument");
    const ImportView view{n_instances ? 1u : 0u, (uint32_t)n->ids.size(), n->ids.data(), n->ids.data(), nullptr};
    ImportPlan checked;
    std::string text;
    if (int rc = import_plan_records(&view, in, records, &checked, &text)) return set_err(rc, text);
    if (in->n_fields && in->pitch > 32u * (uint64_t)n->ids.size())
        return set_err(ACVM_E_INVALID, "pitch " + std::to_string(in->pitch) + " is above 32 * n_initial = " + std::to_string(32u * (uint64_t)n->ids.size()) +
                                           ": the staging slots hold the 32-byte form, and a wider record gains nothing");
    // (the fields are the caller's until the call returns: every lane reads the same array)
    return node_solve_host(n, n_instances, (const uint8_t *)records, in, results, kept_be32, kept_assigned, digests32);
} ABI_CATCH

// The device form: every lane is checked (node_io_plan.cpp) before any lane starts, then each lane's thread walks its own rows.
long long acvm_node_solve_device(acvm_node_t *n, acvm_node_lane_io_t *lanes, uint32_t n_lanes) try {
    if (!n) return set_err(ACVM_E_INVALID, "null argument");
    RunningCall running(n);
    const double t0 = now_ms();
    const size_t D = n->lanes.size();
    std::vector<NodeLaneIo> checked;
    std::string text;
    if (int rc = node_io_check(NodeIoShape{(uint32_t)n->ids.size(), (uint32_t)n->keep.size(), n->tile}, lanes, n_lanes, (uint32_t)D, &checked, &text)) return set_err(rc, text);
    std::vector<std::thread> th;
    for (size_t d = 0; d < D; d++) th.emplace_back(run_lane_device, n, std::ref(n->lanes[d]), std::cref(checked[d]), &lanes[d]);
    for (auto &t : th) t.join();
    uint64_t total = 0;
    for (size_t d = 0; d < D; d++) total += lanes[d].n;
    n->last_n = total;
    n->last_total_ms = now_ms() - t0;
    for (size_t d = 0; d < D; d++)
        if (n->lanes[d].rc) return set_err(n->lanes[d].rc, "lane " + std::to_string(d) + " (device " + std::to_string(n->lanes[d].device) + "): " + n->lanes[d].error);
    long long not_solved = 0;
    for (DeviceLane &L : n->lanes) not_solved += (long long)L.not_solved;
    return not_solved;
} ABI_CATCH
int acvm_debug_node_io_bytes(const acvm_node_t *n, uint32_t lane, uint64_t *h2d, uint64_t *d2h) {
    if (!n || lane >= n->lanes.size()) return set_err(ACVM_E_INVALID, "no such lane");
    if (h2d) *h2d = n->lanes[lane].io_h2d;
    if (d2h) *d2h = n->lanes[lane].io_d2h;
    return 0;
}

int acvm_node_set_foreign_call_handler(acvm_node_t *n, const acvm_node_foreign_handler_t *h) try {
    if (!n) return set_err(ACVM_E_INVALID, "null argument");
    std::string text;
    if (int rc = node_foreign_check_handler(h, n->has_solver, n->running.load() != 0, &text)) return set_err(rc, text);
    n->has_handler = h != nullptr;
    n->handler = h ? *h : acvm_node_foreign_handler_t{};
    return 0;
} ABI_CATCH
int acvm_node_foreign_stats(acvm_node_t *n, uint32_t lane, acvm_node_foreign_stats_t *out) {
    if (!n || !out || lane >= n->lanes.size()) return set_err(ACVM_E_INVALID, !n || !out ? "null argument" : "no such lane");
    *out = n->lanes[lane].fc;
    return 0;
}

int acvm_node_stats(acvm_node_t *n, acvm_node_stats_t *out) {
    if (!n || !out) return set_err(ACVM_E_INVALID, "null argument");
    memset(out, 0, sizeof *out);
    out->n_devices = (uint32_t)n->lanes.size();
    out->tile_instances = n->tile;
    out->n_instances = n->last_n;
    out->total_ms = n->last_total_ms;
    for (size_t d = 0; d < n->lanes.size() && d < 16; d++) {
        const DeviceLane &L = n->lanes[d];
        out->device[d] = L.device;
        out->async_exact[d] = L.async;
        out->tiles[d] = L.tiles;
        out->exact_instances[d] = L.exact_instances;
        out->lane_ms[d] = L.total_ms;
        out->solve_device_ms[d] = L.device_ms;
        out->h2d_wait_ms[d] = L.h2d_wait_ms;
        out->export_ms[d] = L.export_ms;
        out->numa_node[d] = L.numa_node;
        out->n_cpus_pinned[d] = (uint32_t)L.cpus.size();
        out->first_cpu[d] = L.cpus.empty() ? -1 : (int)L.cpus.front();
    }
    out->plans_built = n->plans_built;
    out->create_ms = n->create_ms;
    out->plan_ms = n->plan_ms;
    {   // resident set of the process (the shared plan of a 10^6-opcode circuit is hundreds of MB; it used to exist once per lane)
        std::ifstream f("/proc/self/statm");
        unsigned long long pages_total = 0, pages_resident = 0;
        if (f >> pages_total >> pages_resident) out->host_rss_bytes = (uint64_t)pages_resident * (uint64_t)sysconf(_SC_PAGESIZE);
    }
    return 0;
}

// host-only probes of the placement logic (tests/test_sharding.py: no GPU, a made-up sysfs tree)
int acvm_debug_cpulist(const char *text, uint32_t *cpus, uint32_t cap) try {
    if (!text || (cap && !cpus)) return set_err(ACVM_E_INVALID, "null argument");
    const std::vector<uint32_t> v = parse_cpulist(text);
    for (size_t i = 0; i < v.size() && i < cap; i++) cpus[i] = v[i];
    return (int)v.size();
} ABI_CATCH
int acvm_debug_device_locality(const char *pci_root, const char *bus_id, int *numa_node, uint32_t *cpus, uint32_t cap) try {
    if (!pci_root || !bus_id || !numa_node || (cap && !cpus)) return set_err(ACVM_E_INVALID, "null argument");
    std::vector<uint32_t> v;
    if (!device_locality(pci_root, bus_id, numa_node, &v)) return set_err(ACVM_E_STATE, "no numa_node / local_cpulist for this device");
    for (size_t i = 0; i < v.size() && i < cap; i++) cpus[i] = v[i];
    return (int)v.size();
} ABI_CATCH

}  // extern "C"
