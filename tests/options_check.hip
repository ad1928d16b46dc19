// options_check.hip -- the option table of csrc/hdb_plan.h (HDB_OPTIONS, hdb_option_set) on the host: a stand-alone program, no GPU call.
//
// usage: options_check tests/golden/option_rules.jsonl
// 1) the table: every entry names another member of hdb_options (with the table's static_assert: every member exactly once), and
//    setting an entry changes that member's word of the struct and no other; a name the table does not hold is refused and changes
//    nothing;
// 2) the rules: tests/golden/option_rules.jsonl was recorded from the strcmp ladder hdb_set_option had before the table existed --
//    per line an option's name, a value and the member's value afterwards, starting from the defaults ("first": a value set before
//    it, for the options that ignore what is not in their set).  Every line replays through hdb_option_set; every entry of the table
//    has lines, so an option added later is recorded too.
// Prints "lines N" and " F failures"; exit status 1 on any failure.
#include "plan_check.h"
#include <cstring>
#include <fstream>

static const size_t WORDS = sizeof(hdb_options) / sizeof(int64_t);
static int64_t word(const hdb_options& o, size_t i) { int64_t w; std::memcpy(&w, (const char*)&o + i * sizeof(int64_t), sizeof(w)); return w; }
static size_t word_of(const hdb_options& o, const hdb_option_entry& e) { return (size_t)((const char*)&(o.*e.member) - (const char*)&o) / sizeof(int64_t); }

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: options_check RULES.jsonl\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }
    const hdb_options dflt;

    // ---- 1: the table ----
    bool seen[WORDS] = {};
    for (const hdb_option_entry& e : HDB_OPTIONS) {
        const size_t w = word_of(dflt, e);
        CHECK(w < WORDS && !seen[w], "%s: its member is the member of an entry before it", e.name);
        seen[w] = true;
        long changed = 0;
        for (int64_t v : {(int64_t)-7, (int64_t)0, (int64_t)1, (int64_t)4, (int64_t)32, (int64_t)512, (int64_t)1 << 21}) {
            hdb_options o;
            CHECK(hdb_option_set(o, e.name, v), "%s is refused", e.name);
            for (size_t i = 0; i < WORDS; ++i) if (i != w) CHECK(word(o, i) == word(dflt, i), "%s = %lld changes word %zu", e.name, (long long)v, i);
            if (word(o, w) != word(dflt, w)) ++changed;
        }
        CHECK(changed > 0, "%s: no value changes its member", e.name);
    }
    {
        hdb_options o;
        CHECK(!hdb_option_set(o, "no_such_option", 1) && !hdb_option_set(o, "", 1) && !hdb_option_set(o, "profile", 1), "a name outside the table is refused");
        CHECK(std::memcmp(&o, &dflt, sizeof(o)) == 0, "a refused name changes the options");
    }

    // ---- 2: the recorded rules ----
    std::map<std::string, long> per_name;
    std::string line;
    long lines = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        ++lines;
        Row r;
        if (!parse_row(line, r) || !r.str.count("name") || !r.num.count("value") || !r.num.count("result")) { CHECK(false, "line %ld does not parse", lines); continue; }
        const std::string& name = r.str["name"];
        const hdb_option_entry* e = nullptr;
        for (const hdb_option_entry& t : HDB_OPTIONS) if (name == t.name) e = &t;
        if (!e) { CHECK(false, "line %ld: %s is not in the table", lines, name.c_str()); continue; }
        ++per_name[name];
        hdb_options o;
        if (r.num.count("first")) CHECK(hdb_option_set(o, e->name, r.num["first"]), "line %ld: %s is refused", lines, e->name);
        CHECK(hdb_option_set(o, e->name, r.num["value"]), "line %ld: %s is refused", lines, e->name);
        CHECK(o.*e->member == r.num["result"], "line %ld: %s = %lld gives %lld, the recorded rule gave %lld", lines, e->name, r.num["value"],
              (long long)(o.*e->member), r.num["result"]);
    }
    for (const hdb_option_entry& e : HDB_OPTIONS) CHECK(per_name[e.name] >= 28, "%s has %ld recorded lines", e.name, per_name[e.name]);
    std::printf("lines %ld\n", lines);
    return check_done();
}
