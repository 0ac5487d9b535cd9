// Host check of the code layout (qkd_layout.h): derives the layout of a code and
// prints every scalar and, for every array, its name, kind (d: uploaded, h: kept
// on the host), byte length and FNV-1a 64 hash; with a directory, the arrays'
// bytes too.
//   code_layout_check FILE [bit-order mode | -] [dump directory]
// FILE ("-": stdin): int32 n, m, e, then check_ptr[m + 1] and check_idx[e].
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../qkd_ldpc_amd/csrc/qkd_layout.h"

static char g_error[1024];
qkd_status qkd::set_error(qkd_status s, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return s;
}

static const char* g_dump = nullptr;

template <class T>
static void arr(const char* name, const char* kind, const std::vector<T>& v) {
    const size_t bytes = v.size() * sizeof(T);
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ reinterpret_cast<const unsigned char*>(v.data())[i]) * 0x100000001b3ull;
    printf("a %s %s %zu %016llx\n", name, kind, bytes, (unsigned long long)h);
    if (!g_dump) return;
    FILE* f = fopen((std::string(g_dump) + "/" + name + ".bin").c_str(), "wb");
    if (f) {
        fwrite(v.data(), 1, bytes, f);
        fclose(f);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::string(argv[1]) == "-" ? stdin : fopen(argv[1], "rb");
    int32_t hd[3];
    if (!f || fread(hd, 4, 3, f) != 3 || hd[1] < 0 || hd[2] < 0) return 2;
    std::vector<int32_t> cptr((size_t)hd[1] + 1), cidx(hd[2]);
    if (fread(cptr.data(), 4, cptr.size(), f) != cptr.size() || fread(cidx.data(), 4, cidx.size(), f) != cidx.size())
        return 2;
    const char* mode = argc > 2 && std::string(argv[2]) != "-" ? argv[2] : nullptr;
    g_dump = argc > 3 ? argv[3] : nullptr;
    qkd::CodeLayout L;
    const qkd_status st = qkd::derive_code_layout(hd[0], hd[1], cptr.data(), cidx.data(), mode, false, L);
    printf("status %d %s\n", (int)st, g_error);
    if (st != QKD_OK) return 0;
#define S(x) printf("s %s %lld\n", #x, (long long)L.x)
    S(n); S(m); S(e); S(max_dv); S(max_dc); S(min_dc); S(min_dv); S(is_regular); S(n_pad); S(m_pad); S(n_tasks);
    S(n_pat); S(chk_rs); S(ilv_rs); S(cl_dc); S(keygen_chunk); S(kg_cb); S(kg_cs); S(split);
    for (int k = 0; k < 2; ++k)
        printf("s cl%d_tasks %d\ns cl%d_rem_tasks %d\n", k, L.cl_host[k].cl_tasks, k, L.cl_host[k].rem_tasks);
    arr("check_ptr", "h", L.check_ptr);
    arr("check_idx", "h", L.check_idx);
    arr("bit_ptr", "h", L.bit_ptr);
    arr("bit_idx", "h", L.bit_idx);
    arr("chk_bits", "d", L.chk_bits);
    arr("chk_deg", "d", L.chk_deg);
    arr("chk_odd", "d", L.chk_odd);
    arr("bit_chk", "d", L.bit_chk);
    arr("bit_pos", "d", L.bit_pos);
    arr("bit_deg", "d", L.bit_deg);
    arr("bit_pat", "d", L.bit_pat);
    arr("pat_deg", "dh", L.pat_deg);
    arr("plan", "d", L.plan);
    arr("perm", "dh", L.perm);
    arr("inv", "d", L.inv);
    arr("bit_chk_s", "d", L.bit_chk_s);
    arr("bit_deg_s", "d", L.bit_deg_s);
    arr("bit_pat_s", "d", L.bit_pat_s);
    arr("chk_rows16", "d", L.chk_rows16);
    arr("bit_code", "d", L.bit_code);
    arr("ilv_slots", "d", L.ilv_slots);
    arr("plan_slot", "dh", L.plan_slot);
    for (int k = 0; k < 2; ++k) {
        const std::string p = "cl" + std::to_string(k);
        arr((p + "_slot").c_str(), "h", L.cl_host[k].slot);
        arr((p + "_chk").c_str(), "h", L.cl_host[k].chk);
        arr((p + "_rem").c_str(), "h", L.cl_host[k].rem);
    }
    arr("jump", "d", L.jump);
    arr("jpoly", "d", L.jpoly);
    arr("jpoly2", "d", L.jpoly2);
    return 0;
}
