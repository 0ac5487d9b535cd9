// host.cpp — code objects, matrix readers, errors and host helpers of the
// C ABI (include/qkd_ldpc.h): no kernels. The code's layout is derived in
// qkd_layout.h; the kernels and their launchers live in the .hip files.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <new>
#include <sstream>

#include "qkd_internal.h"
#include "qkd_ntt.h"
#include "qkd_plan.h"
#include "qkd_privacy.h"
#include "qkd_rng.h"
#include "qkd_verify.h"

namespace qkd {

static thread_local std::string g_last_error;

qkd_status set_error(qkd_status s, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return s;
}

void clear_error() { g_last_error.clear(); }

// ---- debug / A-B options (qkd_debug_set_option) -----------------------------
static const char* const kDebugOptions[] = {
    "QKD_SPEC_CAP", "QKD_SPEC_CKPT", "QKD_CKPT_UNSAT", "QKD_SPEC_POLICY", "QKD_FOLD_TABLE",
    "QKD_DECODE_KERNEL", "QKD_MINSUM_STORE", "QKD_DECODE_GRID", "QKD_SPLIT_BUDGET", "QKD_C2B_PAD",
    "QKD_ILV", "QKD_ILV_GRID", "QKD_KEYGEN", "QKD_SYN_SLICED", "QKD_SYN_BYTES", "QKD_BIT_ORDER",
    "QKD_PHASE_TIMING", "QKD_CHECK_LANES", "QKD_PRIVACY_KERNEL", "QKD_PRIVACY_NTT_LOG2"};
static std::mutex g_dbg_mu;                            // guards g_dbg and every workspace's dbg
static std::map<std::string, std::string> g_dbg;

DbgOpt debug_option(const qkd_workspace* ws, const char* name) {
    std::lock_guard<std::mutex> lock(g_dbg_mu);
    DbgOpt o;
    if (ws) {
        const auto it = ws->dbg.find(name);
        if (it != ws->dbg.end()) {
            o.set = true;
            o.v = it->second;
            return o;
        }
    }
    const auto it = g_dbg.find(name);
    if (it != g_dbg.end()) {
        o.set = true;
        o.v = it->second;
    }
    return o;
}

bool debug_options_unset(const qkd_workspace* ws) {
    std::lock_guard<std::mutex> lock(g_dbg_mu);
    return g_dbg.empty() && (!ws || ws->dbg.empty());
}

// Derive the layout (qkd_layout.h), check the device, upload. An array the
// layout leaves empty is not uploaded: its device pointer stays null.
template <class T, class H>
static hipError_t upload(DevBuf<T>& d, const std::vector<H>& v) {
    static_assert(sizeof(T) == sizeof(H), "same element layout");
    return v.empty() ? hipSuccess : d.upload(reinterpret_cast<const T*>(v.data()), v.size());
}

static qkd_status build_code(qkd_code* c, int32_t n, int32_t m, const int32_t* cptr,
                             const int32_t* cidx, int device) {
    CodeLayout L;
    // (QKD_BIT_ORDER: read once, here)
    const DbgOpt bit_order = debug_option(nullptr, "QKD_BIT_ORDER");
    const qkd_status ls = derive_code_layout(n, m, cptr, cidx, bit_order ? bit_order.c_str() : nullptr, false, L);
    if (ls != QKD_OK) return ls;
    c->device = device;
    // what the host keeps: L's CodeHost part moves into the code (so pat_deg,
    // perm and plan_slot are uploaded from there); its other arrays stay in L
    static_cast<CodeHost&>(*c) = std::move(static_cast<CodeHost&>(L));

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_error(QKD_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev)
        return set_error(QKD_ERR_INVALID_ARG, "device %d out of range (%d devices)", device, ndev);
    DeviceGuard g(device);
    QKD_HIP(hipDeviceGetAttribute(&c->cu_count, hipDeviceAttributeMultiprocessorCount, device));
    QKD_HIP(upload(c->d_chk_bits, L.chk_bits));
    QKD_HIP(upload(c->d_chk_deg, L.chk_deg));
    QKD_HIP(upload(c->d_chk_odd, L.chk_odd));
    QKD_HIP(upload(c->d_bit_pos, L.bit_pos));
    QKD_HIP(upload(c->d_bit_chk, L.bit_chk));
    QKD_HIP(upload(c->d_bit_deg, L.bit_deg));
    QKD_HIP(upload(c->d_bit_pat, L.bit_pat));
    QKD_HIP(upload(c->d_pat_deg, c->pat_deg));
    QKD_HIP(upload(c->d_perm, c->perm));
    QKD_HIP(upload(c->d_inv, L.inv));
    QKD_HIP(upload(c->d_chk_rows16, L.chk_rows16));
    QKD_HIP(upload(c->d_bit_chk_s, L.bit_chk_s));
    QKD_HIP(upload(c->d_bit_deg_s, L.bit_deg_s));
    QKD_HIP(upload(c->d_bit_pat_s, L.bit_pat_s));
    QKD_HIP(upload(c->d_bit_code, L.bit_code));
    QKD_HIP(upload(c->d_ilv_slots, L.ilv_slots));
    QKD_HIP(upload(c->d_plan, L.plan));
    QKD_HIP(upload(c->d_plan_slot, c->plan_slot));
    QKD_HIP(upload(c->d_jump, L.jump));
    QKD_HIP(upload(c->d_jpoly, L.jpoly));
    QKD_HIP(upload(c->d_jpoly2, L.jpoly2));
    return QKD_OK;
}

static qkd_code* make_code(int32_t n, int32_t m, const int32_t* cptr, const int32_t* cidx,
                           int device, qkd_status* status) {
    qkd_code* c = new (std::nothrow) qkd_code();
    qkd_status s = c ? build_code(c, n, m, cptr, cidx, device)
                     : set_error(QKD_ERR_OUT_OF_MEMORY, "out of host memory");
    if (s != QKD_OK) {
        delete c;
        c = nullptr;
    }
    if (status) *status = s;
    return c;
}

// ---- readers ---------------------------------------------------------------

// istringstream >> int semantics: integers up to the first non-integer token.
static void parse_ints(const std::string& line, std::vector<long>& out) {
    out.clear();
    const char* s = line.c_str();
    for (;;) {
        while (*s == ' ' || *s == '\t' || *s == '\r' || *s == '\v' || *s == '\f' || *s == '\n') s++;
        if (!*s) break;
        char* end = nullptr;
        errno = 0;
        long v = strtol(s, &end, 10);
        if (end == s || errno == ERANGE || v > INT32_MAX || v < INT32_MIN) break;
        out.push_back(v);
        s = end;
    }
}

static bool read_lines(const char* path, std::vector<std::vector<long>>& rows) {
    std::ifstream f(path);
    if (!f.is_open()) return false;
    std::string line;
    std::vector<long> v;
    while (std::getline(f, line)) {
        parse_ints(line, v);
        rows.push_back(v);
    }
    return true;
}

// read_sparse_alist_matrix (reference array_and_matrix_operations.cpp:109-292)
// sort_rows (QKD_READ_SORT_ROWS): each line's entries are sorted first, so a
// file whose rows are not ascending is read as the matrix it describes instead
// of being rejected (the reference would silently pair messages with the
// wrong edges).
static qkd_status parse_alist(const char* path, int32_t& n, int32_t& m, std::vector<int32_t>& cptr,
                              std::vector<int32_t>& cidx, bool sort_rows) {
    std::vector<std::vector<long>> v;
    if (!path || !read_lines(path, v))
        return set_error(QKD_ERR_IO, "Failed to open file: %s", path ? path : "(null)");
    if (v.empty()) return set_error(QKD_ERR_IO, "File is empty or cannot be read properly: %s", path);
    if (v.size() < 4) return set_error(QKD_ERR_IO, "Insufficient data in the file: %s", path);
    if (v[0].size() != 2 || v[1].size() != 2)
        return set_error(QKD_ERR_IO, "File format does not match the alist format: %s", path);
    const long cols = v[0][0], rows = v[0][1];
    const size_t nb = v[2].size(), nc = v[3].size();
    if (v.size() < 4 + nb + nc) return set_error(QKD_ERR_IO, "Insufficient data in the file: %s", path);
    if (cols != (long)nb)
        return set_error(QKD_ERR_IO, "Number of columns '%ld' is not the same as the length of the third line '%zu'. File: %s", cols, nb, path);
    if (rows != (long)nc)
        return set_error(QKD_ERR_IO, "Number of rows '%ld' is not the same as the length of the fourth line '%zu'. File: %s", rows, nc, path);
    for (size_t i = 0; i < nb + nc; ++i) {
        const auto& L = v[4 + i];
        const long w = i < nb ? v[2][i] : v[3][i - nb];
        long nz = 0;
        for (long x : L) nz += (x != 0);
        if (nz != w || w < 0 || (size_t)w > L.size())
            return set_error(QKD_ERR_IO, "Number of non-zero elements '%ld' in the line '%zu' does not match the weight '%ld'. File: %s", nz, 5 + i, w, path);
    }
    n = (int32_t)cols;
    m = (int32_t)rows;
    // check_nodes rows (the first weight entries of each check line, 1-based)
    cptr.assign(m + 1, 0);
    cidx.clear();
    for (int32_t j = 0; j < m; ++j) {
        const auto& L = v[4 + nb + j];
        for (long k = 0; k < v[3][j]; ++k) cidx.push_back((int32_t)(L[k] - 1));
        if (sort_rows) std::sort(cidx.begin() + cptr[j], cidx.end());
        cptr[j + 1] = (int32_t)cidx.size();
    }
    // bit_nodes rows must describe the same edge set (the reference reads
    // both and would route messages inconsistently if they disagree)
    std::vector<std::vector<int32_t>> from_checks(n);
    for (int32_t j = 0; j < m; ++j)
        for (int32_t k = cptr[j]; k < cptr[j + 1]; ++k) {
            const int32_t b = cidx[k];
            if (b < 0 || b >= n)
                return set_error(QKD_ERR_BAD_CODE, "check %d lists bit %d outside [1,%d]. File: %s", j + 1, b + 1, n, path);
            from_checks[b].push_back(j);
        }
    for (int32_t i = 0; i < n; ++i) {
        const auto& L = v[4 + i];
        std::vector<int32_t> row;
        for (long k = 0; k < v[2][i]; ++k) row.push_back((int32_t)(L[k] - 1));
        if (sort_rows) std::sort(row.begin(), row.end());
        if (row != from_checks[i]) {
            std::vector<int32_t> s = row;
            std::sort(s.begin(), s.end());
            if (s == from_checks[i])
                return set_error(QKD_ERR_UNSORTED, "bit %d: check list not ascending. File: %s", i + 1, path);
            return set_error(QKD_ERR_BAD_CODE, "bit %d: check list disagrees with the check rows. File: %s", i + 1, path);
        }
    }
    return QKD_OK;
}

// read_dense_matrix (reference array_and_matrix_operations.cpp:295-421)
static qkd_status parse_dense(const char* path, int32_t& n, int32_t& m, std::vector<int32_t>& cptr,
                              std::vector<int32_t>& cidx) {
    std::vector<std::vector<long>> v;
    if (!path || !read_lines(path, v))
        return set_error(QKD_ERR_IO, "Failed to open file: %s", path ? path : "(null)");
    if (v.empty()) return set_error(QKD_ERR_IO, "File is empty or cannot be read properly: %s", path);
    for (const auto& r : v)
        for (long x : r)
            if (x != 0 && x != 1)
                return set_error(QKD_ERR_IO, "Parity check matrix can only take values 0 or 1. File: %s", path);
    for (const auto& r : v)
        if (r.size() != v[0].size())
            return set_error(QKD_ERR_IO, "Different lengths of rows in a matrix. File: %s", path);
    n = (int32_t)v[0].size();
    m = (int32_t)v.size();
    for (int32_t i = 0; i < n; ++i) {
        long w = 0;
        for (int32_t j = 0; j < m; ++j) w += v[j][i];
        if (w <= 0)
            return set_error(QKD_ERR_IO, "Column '%d' weight cannot be equal to or less than zero. File: %s", i + 1, path);
    }
    cptr.assign(m + 1, 0);
    cidx.clear();
    for (int32_t j = 0; j < m; ++j) {
        for (int32_t i = 0; i < n; ++i)
            if (v[j][i]) cidx.push_back(i);
        if (cidx.size() == (size_t)cptr[j])
            return set_error(QKD_ERR_IO, "Row '%d' weight cannot be equal to or less than zero. File: %s", j + 1, path);
        cptr[j + 1] = (int32_t)cidx.size();
    }
    return QKD_OK;
}

}  // namespace qkd

using namespace qkd;

extern "C" {

int qkd_abi_version(void) { return QKD_LDPC_ABI_VERSION; }

const char* qkd_last_error(void) { return g_last_error.c_str(); }

const char* qkd_status_string(qkd_status s) {
    switch (s) {
        case QKD_OK: return "ok";
        case QKD_ERR_INVALID_ARG: return "invalid argument";
        case QKD_ERR_BAD_CODE: return "malformed parity-check matrix";
        case QKD_ERR_UNSORTED: return "adjacency row not ascending";
        case QKD_ERR_QBER_TOO_SMALL: return "key size too small for QBER";
        case QKD_ERR_DEVICE: return "HIP device error";
        case QKD_ERR_OUT_OF_MEMORY: return "out of memory";
        case QKD_ERR_IO: return "matrix file error";
        case QKD_ERR_UNSUPPORTED: return "unsupported code shape";
    }
    return "unknown status";
}

int qkd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

qkd_code* qkd_code_create(int32_t n_bits, int32_t n_checks, const int32_t* check_ptr,
                          const int32_t* check_idx, int device, qkd_status* status) {
    clear_error();
    return make_code(n_bits, n_checks, check_ptr, check_idx, device, status);
}

qkd_code* qkd_code_from_alist(const char* path, int device, qkd_status* status) {
    return qkd_code_from_alist_ex(path, device, 0, status);
}

qkd_code* qkd_code_from_alist_ex(const char* path, int device, uint32_t read_flags, qkd_status* status) {
    clear_error();
    if (read_flags & ~QKD_READ_SORT_ROWS) {
        set_error(QKD_ERR_INVALID_ARG, "unknown read flags 0x%x", read_flags);
        if (status) *status = QKD_ERR_INVALID_ARG;
        return nullptr;
    }
    int32_t n = 0, m = 0;
    std::vector<int32_t> cptr, cidx;
    qkd_status s = parse_alist(path, n, m, cptr, cidx, (read_flags & QKD_READ_SORT_ROWS) != 0);
    if (s != QKD_OK) {
        if (status) *status = s;
        return nullptr;
    }
    return make_code(n, m, cptr.data(), cidx.data(), device, status);
}

qkd_code* qkd_code_from_dense(const char* path, int device, qkd_status* status) {
    clear_error();
    int32_t n = 0, m = 0;
    std::vector<int32_t> cptr, cidx;
    qkd_status s = parse_dense(path, n, m, cptr, cidx);
    if (s != QKD_OK) {
        if (status) *status = s;
        return nullptr;
    }
    return make_code(n, m, cptr.data(), cidx.data(), device, status);
}

qkd_status qkd_debug_set_option(qkd_workspace* ws, const char* name, const char* value) {
    clear_error();
    if (!name) return set_error(QKD_ERR_INVALID_ARG, "option name is null");
    bool known = false;
    for (const char* k : kDebugOptions) known = known || !strcmp(k, name);
    if (!known) return set_error(QKD_ERR_INVALID_ARG, "unknown debug option '%s'", name);
    std::lock_guard<std::mutex> lock(g_dbg_mu);
    std::map<std::string, std::string>& m = ws ? ws->dbg : g_dbg;
    if (value) m[name] = value;
    else m.erase(name);
    return QKD_OK;
}

void qkd_code_destroy(qkd_code* code) {
    if (!code) return;
    if (code->default_ws) qkd_workspace_destroy(code->default_ws);
    delete code;
}

qkd_status qkd_code_get_info(const qkd_code* c, qkd_code_info* info) {
    if (!c || !info) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    info->n_bits = c->n;
    info->n_checks = c->m;
    info->n_edges = c->e;
    info->max_bit_degree = c->max_dv;
    info->max_check_degree = c->max_dc;
    info->is_regular = c->is_regular;
    info->device = c->device;
    return QKD_OK;
}

qkd_status qkd_code_get_adjacency(const qkd_code* c, int32_t* check_ptr, int32_t* check_idx,
                                  int32_t* bit_ptr, int32_t* bit_idx) {
    if (!c) return set_error(QKD_ERR_INVALID_ARG, "null code");
    if (check_ptr) std::memcpy(check_ptr, c->check_ptr.data(), c->check_ptr.size() * 4);
    if (check_idx) std::memcpy(check_idx, c->check_idx.data(), c->check_idx.size() * 4);
    if (bit_ptr) std::memcpy(bit_ptr, c->bit_ptr.data(), c->bit_ptr.size() * 4);
    if (bit_idx) std::memcpy(bit_idx, c->bit_idx.data(), c->bit_idx.size() * 4);
    return QKD_OK;
}

qkd_status qkd_debug_bit_order(int32_t n, int32_t m, const int32_t* cptr, const int32_t* cidx, const char* mode,
                               int32_t* perm_out, uint32_t* plan_out, int32_t* n_tasks_out) {
    clear_error();
    if (!n_tasks_out) return set_error(QKD_ERR_INVALID_ARG, "bad arguments");
    // (the layout's validation first: the sizes below come from cptr)
    CodeLayout L;
    const qkd_status ls = derive_code_layout(n, m, cptr, cidx, mode, true, L);
    if (ls != QKD_OK) return ls;
    if (perm_out) std::copy(L.perm.begin(), L.perm.end(), perm_out);
    if (plan_out)
        for (size_t k = 0; k < (size_t)L.n_tasks * 64; ++k) plan_out[k] = L.plan[k].x;
    *n_tasks_out = L.n_tasks;
    return QKD_OK;
}

qkd_status qkd_adapt_positions(int32_t n, int32_t m, const int32_t* cptr, const int32_t* cidx, int32_t count,
                               uint64_t seed, int32_t* positions, int32_t* untainted_out) {
    clear_error();
    std::vector<int32_t> bdeg;
    int32_t max_dc = 0;
    const qkd_status vs = validate_csr(n, m, cptr, cidx, bdeg, max_dc);
    if (vs != QKD_OK) return vs;
    if (count < 0 || count > n || (count > 0 && !positions))
        return set_error(QKD_ERR_INVALID_ARG, "qkd_adapt_positions: count %d outside [0, %d] or null output", count, n);
    // the candidates' order: Fisher-Yates from the top, draw k = R[k] of the seeded string
    std::vector<int32_t> order(n);
    for (int32_t i = 0; i < n; ++i) order[i] = i;
    uint64_t k = 0;
    for (int32_t i = n - 1; i >= 1; --i, ++k) {
        const uint64_t j = qkdv::verify_key_word(seed, k) % (uint64_t)(i + 1);
        std::swap(order[i], order[(size_t)j]);
    }
    // bit-side lists: the checks of each bit
    std::vector<int32_t> bptr, bidx;
    bit_side_lists(n, m, cptr, cidx, bdeg, bptr, bidx, nullptr);
    // pass 1: candidates none of whose checks touches an earlier pick
    std::vector<uint8_t> tainted(m, 0), taken(n, 0);
    int32_t got = 0;
    for (int32_t t = 0; t < n && got < count; ++t) {
        const int32_t b = order[t];
        bool free_ = true;
        for (int32_t e = bptr[b]; e < bptr[b + 1]; ++e) free_ = free_ && !tainted[bidx[e]];
        if (!free_) continue;
        for (int32_t e = bptr[b]; e < bptr[b + 1]; ++e) tainted[bidx[e]] = 1;
        taken[b] = 1;
        positions[got++] = b;
    }
    if (untainted_out) *untainted_out = got;
    // pass 2: the untaken candidates in the same order
    for (int32_t t = 0; t < n && got < count; ++t) {
        const int32_t b = order[t];
        if (taken[b]) continue;
        taken[b] = 1;
        positions[got++] = b;
    }
    return QKD_OK;
}

qkd_status qkd_make_seeds(uint64_t simulation_seed, size_t count, uint64_t* seeds) {
    if (count && !seeds) return set_error(QKD_ERR_INVALID_ARG, "null seeds");
    qkdr::Xoshiro256pp g;
    g.seed(simulation_seed);
    for (size_t i = 0; i < count; ++i) seeds[i] = g.next();
    return QKD_OK;
}

size_t qkd_verify_key_words(int32_t n_bits) { return qkdv::verify_key_words(n_bits); }

qkd_status qkd_verify_expand_key(uint64_t hash_seed, int32_t n_bits, uint64_t* words_host) {
    clear_error();
    if (!words_host) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    if (n_bits < 1) return set_error(QKD_ERR_INVALID_ARG, "n_bits must be > 0");
    const size_t w = qkdv::verify_key_words(n_bits);
    for (size_t k = 0; k < w; ++k) words_host[k] = qkdv::verify_key_word(hash_seed, k);
    return QKD_OK;
}

size_t qkd_privacy_key_words(uint32_t n_in, uint32_t out_bits) { return qkdv::privacy_key_words(n_in, out_bits); }

qkd_status qkd_privacy_expand_key(uint64_t hash_seed, uint32_t n_in, uint32_t out_bits, uint64_t* words_host) {
    clear_error();
    if (!words_host) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    const size_t w = qkdv::privacy_key_words(n_in, out_bits);
    if (w == 0) return set_error(QKD_ERR_INVALID_ARG, "need 1 <= out_bits <= n_in <= QKD_PRIVACY_MAX_BITS");
    for (size_t k = 0; k < w; ++k) words_host[k] = qkdv::verify_key_word(hash_seed, k);
    return QKD_OK;
}

size_t qkd_privacy_long_key_words(uint32_t n_in, uint32_t out_bits) { return qkdn::long_key_words(n_in, out_bits); }

qkd_status qkd_privacy_long_expand_key(uint64_t hash_seed, uint32_t n_in, uint32_t out_bits, uint64_t* words_host) {
    clear_error();
    if (!words_host) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    const size_t w = qkdn::long_key_words(n_in, out_bits);
    if (w == 0)
        return set_error(QKD_ERR_INVALID_ARG,
                         "need 1 <= out_bits <= n_in and n_in + out_bits - 1 <= QKD_PRIVACY_LONG_MAX_BITS");
    for (size_t k = 0; k < w; ++k) words_host[k] = qkdv::verify_key_word(hash_seed, k);
    return QKD_OK;
}

qkd_status qkd_qber_range(double begin, double end, double step, double* values, size_t capacity,
                          size_t* count) {
    if (!count || !(step > 0.0)) return set_error(QKD_ERR_INVALID_ARG, "bad QBER range");
    const double r = std::round((end - begin) / step);
    const size_t steps = r > 0 ? (size_t)r : 0;
    for (size_t j = 0; j < steps && j < capacity && values; ++j) values[j] = begin + (double)j * step;
    *count = steps;
    return QKD_OK;
}

}  // extern "C"
