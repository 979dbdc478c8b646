// Prints the dispatch table of the library as csrc/rotation_plan.hpp states it - no GPU, no library: the header alone.
// tests/test_rotation_plan.py compares the output with tests/rotation_plan_cases.txt; tests/test_gpu_rotation_plan.py drives the
// real library through the same lines.
//
// One `ctx` line per context shape (modulus, log_N, l, Bg; every parameter set has n = 8, which dispatch does not look at): the
// shapes bmi_ctx_create admits and a few it refuses.  Under an admitted shape one `seq` per sequence of calls on a fresh context
// (the setters, what the context answers without keys, key generation, what it answers with keys);
// a step is `<call> -> ok ...` or `<call> -> REFUSED: <the text of bmi_last_error>`, and a refused call changes nothing.
//   unroll F / precision B    bmi_set_bsk_unroll / bmi_set_bsk_precision; ok prec=<bmi_get_bsk_precision afterwards>
//   keygen                    the key copies on the device afterwards and their bytes (bmi_key_bytes)
//   variant V,..              bmi_set_kernel_variant for each V, then per batch size bmi_rotation_kernel's answer
//                             (`*` = every batch size of 1 256 257 512 513 1025); variants that answer alike share a line
//   margin V,..               the kernel of bmi_fft_margin_host under those variants (contexts with keys)
//   import_unrolled           bmi_import_bsk_unrolled's verdict, last: an accepted key replaces the unrolled key
//   import_unrolled_seeded    the shape and precision checks of bmi_import_bsk_unrolled_seeded (after a seeded key set)
//   same as <seq> #i          the context is in the state that sequence was in at its i-th block of variant .. import_unrolled
//                             lines: that block applies here
//
// Beside the printing, the rows of the plan (ROT_ROWS, COPY_ROWS) are held to the plan itself: at every `variant` and `margin`
// answer the kernel's key copy must be held (or built on demand) and its tables among those a context of that shape uploads; so
// must the tables of every copy's converter; and the accumulator and statistics flags must be the lists below.  A miss is
// reported on stderr, and the program then ends with status 1 and the number of misses.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../bounty-matrix-inversion_amd/csrc/rotation_plan.hpp"

using namespace rotplan;

static const uint32_t N_LWE = 8;
static const uint32_t COUNTS[] = {1, 256, 257, 512, 513, 1025};
static const uint32_t PRECISIONS[] = {64, 48, 46, 44, 42, 40};

static const char *modulus_name(Modulus m) { return m == Modulus::torus64 ? "torus64" : m == Modulus::field49 ? "field49" : "goldilocks"; }

struct Ctx {
    Shape shape;
    Settings set;
    Held held;
};

static int misses = 0;
static void expect(bool ok, const Ctx &c, const char *who, const char *what) {
    if (ok) return;
    misses++;
    fprintf(stderr, "MISS %s logN=%u l=%u Bg=%u prec=%d unroll=%u: %s %s\n", modulus_name(c.shape.modulus), c.shape.log_N, c.shape.bs_levels,
            c.shape.bs_base_log, c.set.bsk_prec, c.set.unroll, who, what);
}
// a kernel the plan answered with: launch_rotation must find its key copy and its tables on the device (a context without keys
// names its kernel too, to bmi_rotation_kernel, but every entry point that launches refuses it before: no copy to ask for)
static void check_answer(const Ctx &c, Rot rot) {
    const RotRow &r = row(rot);
    expect(!c.held.have_keys || c.held.has(r.key) || (on_demand_copies(rot) & bit(r.key)) != 0, c, r.name,
           "reads a key copy that is neither held nor built on demand");
    for (Table t : r.tab) expect((bit(t) & ~context_tables(c.shape)) == 0, c, r.name, "names a table that the context does not upload");
}
// the copies held: their converters ran on tables of the context
static void check_copies(const Ctx &c) {
    for (int k = 0; k < (int)Copy::COUNT; k++)
        for (Table t : row((Copy)k).tab)
            expect(!c.held.has((Copy)k) || (bit(t) & ~context_tables(c.shape)) == 0, c, copy_name((Copy)k), "is converted with a table that the context does not upload");
}
// the flags, against the lists the switches of launch_rotation and has_accumulator_form spelled out before the rows existed
static void check_flags() {
    const Rot accumulator[] = {Rot::t64_wide_u, Rot::t64_wide_u2, Rot::t64_wide2, Rot::t64_wide, Rot::t64_quad, Rot::t64_tp2u_fft, Rot::t64_lat2u_fft,
                               Rot::t64_lat_fft, Rot::t64_fft};
    const Rot stat[] = {Rot::t64_wide_u, Rot::t64_wide_u2, Rot::t64_wide, Rot::t64_quad, Rot::t64_lat2u_fft, Rot::t64_lat_fft, Rot::t64_fft};
    const Ctx none{Shape{Modulus::goldilocks, 0, 0, 0}, Settings{0, false, 0, 0, 0}, Held{0, false, false}};
    // ... and the key copy and tables each case of that switch handed its launcher.  (Holding a copy is not enough to tell two
    // copies apart that are always built together, such as fft and fft_lat: a row naming the wrong one of them passes check_answer.)
    const Table no = Table::none;
    const struct { Rot rot; Copy key; Table tab[3]; } wiring[] = {
        {Rot::t64_wide_u, Copy::u_wide, {Table::tw_quarter, Table::zeta_oct, no}}, {Rot::t64_wide_u2, Copy::u_wide, {Table::tw_quarter, Table::zeta_oct, no}},
        {Rot::t64_wide2, Copy::wide2, {Table::tw_quarter, no, no}}, {Rot::t64_wide, Copy::wide, {Table::tw_quarter, no, no}},
        {Rot::t64_quad, Copy::quad, {Table::tw_eighth, no, no}}, {Rot::t64_tp2u_fft, Copy::u_fft_lat, {Table::tw_fft_half, Table::zeta_pow, no}},
        {Rot::t64_lat2u_fft, Copy::u_fft_lat, {Table::tw_fft_half, Table::zeta_pow, no}}, {Rot::t64_lat2u, Copy::u_exact_lat, {Table::tw_half, Table::root_pow, no}},
        {Rot::t64_lat_fft, Copy::fft_lat, {Table::tw_fft_half, no, no}}, {Rot::t64_lat, Copy::exact_lat, {Table::tw_half, no, no}},
        {Rot::t64_fft, Copy::fft, {Table::tw_fft, no, no}}, {Rot::t64_exact, Copy::exact, {Table::tw_wave, no, no}},
        {Rot::f49_wide_u, Copy::u_wide49, {Table::tw_wave, Table::tw_wide49, Table::root_pow}}, {Rot::f49_wide, Copy::wide49, {Table::tw_wave, Table::tw_wide49, no}},
        {Rot::f49_quad, Copy::quad49, {Table::tw_wave, Table::tw_quad49, no}}, {Rot::f49_lat2u, Copy::u_lat49, {Table::tw_half, Table::root_pow, no}},
        {Rot::f49_lat2, Copy::lat49, {Table::tw_half, no, no}}, {Rot::f49_tpx, Copy::ntt49, {Table::tw_wave, no, no}},
        {Rot::gl_lat, Copy::ntt_gl, {Table::tw_gl, no, no}}, {Rot::gl_tp, Copy::ntt_gl, {Table::tw_gl, no, no}}};
    static_assert(sizeof(wiring) / sizeof(wiring[0]) == (size_t)Rot::COUNT, "one case per kernel");
    for (const auto &w : wiring) {
        const RotRow &r = row(w.rot);
        expect(r.key == w.key, none, r.name, "reads another key copy than its launcher was handed");
        expect(r.tab[0] == w.tab[0] && r.tab[1] == w.tab[1] && r.tab[2] == w.tab[2], none, r.name, "reads other tables than its launcher was handed");
    }
    for (int k = 0; k < (int)Rot::COUNT; k++) {
        bool acc = false, st = false;
        for (Rot r : accumulator) acc = acc || r == (Rot)k;
        for (Rot r : stat) st = st || r == (Rot)k;
        expect(has_accumulator_form((Rot)k) == acc, none, rotation_name((Rot)k), "has the wrong accumulator flag");
        expect(row((Rot)k).stat == st, none, rotation_name((Rot)k), "has the wrong statistics flag");
    }
}

static std::string verdict(const std::string &refusal, const std::string &ok) { return refusal.empty() ? ok : "REFUSED: " + refusal; }

static uint64_t copies_bytes(const Ctx &c) {
    const uint64_t limbs = c.shape.t64() ? (uint64_t)t64::limbs_of(c.set.bsk_prec) : 1;
    const uint64_t poly_words = (uint64_t)2 * c.shape.bs_levels * 2 << c.shape.log_N;   // one GGSW: (k + 1) l rows of k + 1 polynomials
    uint64_t bytes = 0;
    for (int k = 0; k < (int)Copy::COUNT; k++)
        if (c.held.has((Copy)k)) bytes += (row((Copy)k).unrolled ? (N_LWE + 1) / 2 * 3 : N_LWE) * poly_words * 8 * limbs;
    return bytes;
}

static void print_keys(const char *step, const Ctx &c) {
    std::string names;
    for (int k = 0; k < (int)Copy::COUNT; k++)
        if (c.held.has((Copy)k)) names += (names.empty() ? "" : ",") + std::string(copy_name((Copy)k));
    check_copies(c);
    printf("  %s -> copies=%s bytes=%llu\n", step, names.empty() ? "none" : names.c_str(), (unsigned long long)copies_bytes(c));
}

static void do_unroll(Ctx &c, uint32_t factor) {
    const UnrollChoice ch = set_unroll(c.shape, c.set, c.held, factor);
    if (ch.refusal.empty()) {
        c.set.bsk_prec = ch.bsk_prec;
        c.set.unroll = factor;
    }
    printf("  unroll %u -> %s\n", factor, verdict(ch.refusal, "ok prec=" + std::to_string(c.shape.t64() ? c.set.bsk_prec : 64)).c_str());
    if (ch.refusal.empty() && factor == 2 && c.held.have_keys && !c.held.have_bsk3) {   // the unrolled key of the secret keys held, at once
        c.held.copies |= unrolled_copies(c.shape, c.set.bsk_prec);
        c.held.have_bsk3 = true;
        print_keys("keys", c);
    }
}

static void do_precision(Ctx &c, uint32_t bits) {
    const std::string refusal = set_precision_refusal(c.shape, c.set, c.held, bits);
    if (refusal.empty()) {
        c.set.bsk_prec = (int)bits;
        c.set.bsk_prec_explicit = true;
    }
    printf("  precision %u -> %s\n", bits, verdict(refusal, "ok prec=" + std::to_string(c.set.bsk_prec)).c_str());
}

static void do_keygen(Ctx &c) {
    c.held.copies = plain_copies(c.shape, c.set.bsk_prec) | (c.set.unroll == 2 ? unrolled_copies(c.shape, c.set.bsk_prec) : 0);
    c.held.have_keys = true;
    c.held.have_bsk3 = c.set.unroll == 2;
    print_keys("keygen", c);
}

// the answers for the six batch sizes on one line
template <class Rule>
static std::string per_count(const Ctx &c, Rule rule) {
    std::vector<std::string> ans;
    for (uint32_t n : COUNTS) {
        const Choice ch = rule(c.shape, c.set, c.held, n);
        if (ch.refusal.empty()) check_answer(c, ch.rot);
        ans.push_back(verdict(ch.refusal, rotation_name(ch.rot)));
    }
    bool same = true;
    for (const std::string &a : ans) same = same && a == ans[0];
    if (same) return "* = " + ans[0];
    std::string line;
    for (size_t i = 0; i < ans.size(); i++) line += (i ? " ; " : "") + std::to_string(COUNTS[i]) + " = " + ans[i];
    return line;
}

// what remains to be said once the setters and the key generation are done
static void tail(Ctx c) {
    std::vector<std::pair<std::string, std::string>> kernel, margin;   // (answers, variants)
    auto add = [](std::vector<std::pair<std::string, std::string>> &rows, const std::string &ans, int v) {
        for (auto &r : rows)
            if (r.first == ans) {
                r.second += "," + std::to_string(v);
                return;
            }
        rows.push_back({ans, std::to_string(v)});
    };
    for (int v = -1; v <= 7; v++) {
        const std::string refusal = set_variant_refusal(c.shape, v);
        if (!refusal.empty()) {
            add(kernel, "REFUSED: " + refusal, v);
            continue;
        }
        c.set.variant = v;
        add(kernel, per_count(c, choose_rotation), v);
        if (c.held.have_keys) add(margin, per_count(c, margin_rotation), v);
    }
    c.set.variant = 0;
    for (const auto &r : kernel) printf("  variant %s -> %s\n", r.second.c_str(), r.first.c_str());
    for (const auto &r : margin) printf("  margin %s -> %s\n", r.second.c_str(), r.first.c_str());
    printf("  import_unrolled_seeded -> %s\n", verdict(import_unrolled_seeded_refusal(c.shape, c.set), "ok").c_str());
    printf("  import_unrolled -> %s\n", verdict(import_unrolled_refusal(c.shape, c.set, c.held), "ok").c_str());
}

static std::map<std::string, std::string> seen;   // state after the setters and key generation -> the sequence that printed its tail

static void finish(const std::string &name, const Ctx &c) {
    char key[96];
    snprintf(key, sizeof key, "%d %u %x %d %d", c.set.bsk_prec, c.set.unroll, c.held.copies, (int)c.held.have_keys, (int)c.held.have_bsk3);
    const auto it = seen.find(key);
    if (it != seen.end()) {
        printf("  same as %s\n", it->second.c_str());
        return;
    }
    seen[key] = name;
    tail(c);
}

static void context(Modulus m, uint32_t log_N, uint32_t l, uint32_t bg) {
    const Shape s{m, log_N, l, bg};
    std::string refusal = ring_refusal(s);
    if (refusal.empty()) refusal = decomposition_refusal(s);
    printf("ctx %s logN=%u l=%u Bg=%u -> %s\n", modulus_name(m), log_N, l, bg, verdict(refusal, "ok").c_str());
    if (!refusal.empty()) return;
    seen.clear();
    const Ctx fresh{s, initial_settings(s), Held{0, false, false}};
    for (uint32_t u = 1; u <= 2 && !s.t64(); u++) {   // the prime fields refuse every precision, and a refused call changes nothing:
        const std::string name = "unroll=" + std::to_string(u) + " precision=every value before and after";   // one context hears them all
        printf(" seq %s\n", name.c_str());
        Ctx c = fresh;
        for (uint32_t bits : PRECISIONS) do_precision(c, bits);
        do_unroll(c, u);
        for (uint32_t bits : PRECISIONS) do_precision(c, bits);
        finish(name + " #1", c);
        do_keygen(c);
        finish(name + " #2", c);
    }
    for (uint32_t u = 1; u <= 2 && s.t64(); u++)
        for (int p = -1; p < 12; p++) {   // precision unset, then each value before and after the unrolling factor
            const uint32_t bits = p < 0 ? 0 : PRECISIONS[p / 2];
            const bool before = p >= 0 && p % 2 == 0;
            const std::string name = "unroll=" + std::to_string(u) + (p < 0 ? " precision=unset" : " precision=" + std::to_string(bits) + (before ? ":before" : ":after"));
            printf(" seq %s\n", name.c_str());
            Ctx c = fresh;
            if (before) do_precision(c, bits);
            do_unroll(c, u);
            if (p >= 0 && !before) do_precision(c, bits);
            finish(name + " #1", c);   // without keys,
            do_keygen(c);
            finish(name + " #2", c);   // and with them
        }
    for (uint32_t u = 1; u <= 2; u++) {   // the factor changed on a context that holds keys
        const std::string name = "unroll=" + std::to_string(3 - u) + " keygen then unroll=" + std::to_string(u);
        printf(" seq %s\n", name.c_str());
        Ctx c = fresh;
        do_unroll(c, 3 - u);
        do_keygen(c);
        do_unroll(c, u);
        finish(name + " #1", c);
    }
}

int main() {
    const Modulus G = Modulus::goldilocks, F = Modulus::field49, T = Modulus::torus64;
    // every shape bmi_ctx_create admits ...
    context(G, 10, 3, 15);
    for (uint32_t log_N = 10; log_N <= 11; log_N++) {
        context(F, log_N, 3, 15);
        context(F, log_N, 2, 15);
        context(F, log_N, 1, 23);
    }
    context(F, 12, 3, 15);
    for (uint32_t l = 3; l >= 2; l--) context(T, 10, l, 10);
    for (uint32_t l = 3; l >= 2; l--) context(T, 10, l, 15);
    for (uint32_t log_N = 11; log_N <= 12; log_N++)
        for (uint32_t l = 3; l >= 2; l--) context(T, log_N, l, 10);
    // ... and one per branch that refuses
    context(T, 9, 3, 10);     // ring size below / above the range
    context(F, 13, 3, 15);
    context(G, 11, 3, 15);    // Goldilocks beyond N = 1024
    context(G, 10, 2, 15);    // decompositions: Goldilocks takes (3, 2^15) only
    context(F, 12, 2, 15);    // the 49-bit field at N = 4096 too
    context(F, 10, 1, 15);    // no such pair on the 49-bit field
    context(T, 10, 1, 23);    // nor on the torus at N = 1024 (default precision 64 at this base)
    context(T, 10, 4, 10);
    context(T, 11, 3, 15);    // N = 2048 / 4096 on the torus: base 2^10 only
    context(T, 12, 3, 15);
    check_flags();
    if (misses) fprintf(stderr, "%d checks of the rows missed\n", misses);
    return misses ? 1 : 0;
}
