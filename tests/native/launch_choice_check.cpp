// Host check of the decode launch's decision (qkd_launch.h choose_decode):
// derives the layout of a code, fills CodeFacts from it and prints every field
// of the DecodeChoice of each case.
//   launch_choice_check CODE CASES
// CODE ("-": none, the cases give every fact): int32 n, m, e, then
// check_ptr[m + 1] and check_idx[e]. CASES: one case per line,
//   NAME key=value ...
// keys: CodeFacts fields (override the derived ones), LaunchFacts fields,
// LaunchOptions fields (an OptInt by its name: set to the value), allow_ilv.
// first_table=auto / tab2=auto: what decode_keys (api.hip) gives the launch.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

#include "../../qkd_ldpc_amd/csrc/qkd_launch.h"

static char g_error[1024];
qkd_status qkd::set_error(qkd_status s, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return s;
}

using namespace qkd;

static void key(const char* name, const KernelKey& k) {
    static const char* kinds[] = {"none", "classic", "split", "ilv"};
    printf(" %s=%s:%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", name, kinds[k.kind], k.mode, k.rule, k.dc, (int)k.clamp,
           (int)k.gt, k.spec, (int)k.lng, (int)k.era, (int)k.vfy, k.rs, (int)k.tg, (int)k.ug);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    CodeFacts base;
    if (std::string(argv[1]) != "-") {
        FILE* f = fopen(argv[1], "rb");
        int32_t hd[3];
        if (!f || fread(hd, 4, 3, f) != 3 || hd[1] < 0 || hd[2] < 0) return 2;
        std::vector<int32_t> cptr((size_t)hd[1] + 1), cidx(hd[2]);
        if (fread(cptr.data(), 4, cptr.size(), f) != cptr.size() || fread(cidx.data(), 4, cidx.size(), f) != cidx.size())
            return 2;
        fclose(f);
        CodeLayout L;
        if (derive_code_layout(hd[0], hd[1], cptr.data(), cidx.data(), nullptr, false, L) != QKD_OK) {
            fprintf(stderr, "layout: %s\n", g_error);
            return 3;
        }
        base = code_facts(L, 256);
    }
    std::ifstream in(argv[2]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string name, kv;
        if (!(ss >> name) || name[0] == '#') continue;
        std::map<std::string, std::string> v;
        while (ss >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) return 2;
            v[kv.substr(0, eq)] = kv.substr(eq + 1);
        }
        const auto has = [&](const char* k) { return v.count(k) != 0; };
        const auto num = [&](const char* k, long d) { return has(k) ? atol(v[k].c_str()) : d; };
        const auto opt = [&](const char* k) {
            OptInt o;
            o.set = has(k);
            o.v = num(k, 0);
            return o;
        };
        CodeFacts c = base;
#define CF(x) c.x = (decltype(c.x))num(#x, (long)c.x)
        CF(n); CF(m); CF(n_pad); CF(max_dv); CF(max_dc); CF(n_pat); CF(n_tasks); CF(cl_dc); CF(ilv_rs);
        CF(has_bit_code); CF(has_ilv_slots); CF(cu_count);
#undef CF
        c.cl_tasks[0] = (int32_t)num("cl0_tasks", c.cl_tasks[0]);
        c.cl_rem_tasks[0] = (int32_t)num("cl0_rem_tasks", c.cl_rem_tasks[0]);
        c.cl_tasks[1] = (int32_t)num("cl1_tasks", c.cl_tasks[1]);
        c.cl_rem_tasks[1] = (int32_t)num("cl1_rem_tasks", c.cl_rem_tasks[1]);
        LaunchFacts f;
        f.mode = (int)num("mode", kModeKeys);
        f.flags = (uint32_t)num("flags", QKD_FLAG_THRESHOLD);
        f.n_frames = (uint32_t)num("n_frames", 1024);
        f.clamp_on = (f.flags & QKD_FLAG_THRESHOLD) != 0;
        f.spec_cap = (uint32_t)num("spec_cap", 0);
        f.ckpt_unsat = (uint32_t)num("ckpt_unsat", 0);
        const int rule = rule_of(f.flags);
        f.first_table = v["first_table"] == "auto" ? (c.max_dc <= kFirstTableDeg ? 1 : 0) : (int)num("first_table", 0);
        f.tab2_entries = v["tab2"] == "auto"
                             ? (f.first_table && c.n_pat > 0 && rule == kRuleSp64 ? c.n_pat * tab2_stride(c.max_dv) : 0)
                             : (int)num("tab2", 0);
        f.trace = num("trace", 0) != 0;
        f.bits_out = num("bits_out", 0) != 0;
        f.class_verify = num("vfy", 0) != 0;
        f.adapt = num("adapt", 0) != 0;
        LaunchOptions o;
        o.ms_global = num("ms_global", 0) != 0;
        o.ms_lds = num("ms_lds", 0) != 0;
        o.classic = num("classic", 0) != 0;
        if (has("budget")) o.split_budget = (size_t)num("budget", 0) < kLdsBytesMax ? (size_t)num("budget", 0) : kLdsBytesMax;
        o.fold_table = opt("fold_table");
        o.spec_always = num("spec_always", 0) != 0;
        o.check_lanes = opt("check_lanes");
        o.c2b_pad = opt("c2b_pad");
        o.ilv = opt("ilv");
        const DecodeChoice ch = choose_decode(c, f, o, num("allow_ilv", 1) != 0);
        printf("%s status=%d", name.c_str(), (int)ch.status);
        if (ch.status != QKD_OK) {
            printf(" message=%s\n", ch.message);
            continue;
        }
        printf(" path=%d rule=%d bucket=%d", ch.path, ch.rule, ch.bucket);
        key("decoder", ch.decoder);
        key("ilv", ch.ilv);
        key("handoff", ch.handoff);
        printf(" lds_bytes=%zu split_bytes=%zu split_S=%u split_msg=%zu ilv_bytes=%zu lds_budget=%u esz=%d",
               ch.lds_bytes, ch.split.bytes, ch.split.S, ch.split.msg, ch.ilv_lds.bytes, ch.lds_budget, ch.esz);
        printf(" ftab_entries=%d spec=%d ckpt=%d spec_always=%d cl_form=%d cl_tasks=%d cl_rem_tasks=%d cl_split=%u"
               " cl_report=%d", ch.ftab_entries, (int)ch.spec, (int)ch.ckpt, (int)ch.spec_always, ch.cl_form, ch.cl_tasks,
               ch.cl_rem_tasks, ch.cl_split, (int)ch.cl_report);
        printf(" c2b_stride=%zu istride=%zu tsg=%d ug=%d gt=%d ilv_forced=%d dead_ok=%d", ch.c2b_stride, ch.istride,
               (int)ch.tsg, (int)ch.ug, (int)ch.gt, (int)ch.ilv_forced, (int)ch.dead_ok);
        printf(" need_c2b=%d need_plan=%d need_ckpt=%d need_ilv=%d win_count=%u spec_cap=%u first_table=%d tab2_entries=%d",
               (int)ch.need_c2b, (int)ch.need_plan, (int)ch.need_ckpt, (int)ch.need_ilv, ch.win_count, ch.spec_cap,
               ch.first_table, ch.tab2_entries);
        // derived, for the structural conditions
        printf(" slots=%zu kC2bPad=%zu kLdsBytesMax=%zu dead_check=%d", c.slots(), kC2bPad, kLdsBytesMax,
               (int)slot_dead_ok(ch.split.bytes, ch.c2b_stride));
        // the facts the LDS layouts are functions of
        printf(" n=%d m=%d n_pad=%d max_dv=%d tab2_in=%d sc=%d\n", c.n, c.m, c.n_pad, c.max_dv, f.tab2_entries,
               (int)((f.flags & QKD_MINSUM_SELF_CORRECT) != 0));
    }
    return 0;
}
