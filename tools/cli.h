// cli.h -- what the executables of tools/ share: how a tool fails, how an option is matched and its number read, owning
// handles of the library's objects, and the mask / record plumbing between a DAZZ_DB on disk and a library call.
// Header-only, plain C++17.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../include/dentist_hip.h"

// ---------------------------------------------------------------------------------- failing
// `<tool>: <msg>` on stderr (the message alone while g_tool is empty) and exit: no destructor of the caller runs, stdio is
// flushed.  die: the usage exits (1).  fail: what goes wrong behind the options (2).  CHK: a library call whose message is
// prefixed with the call's text and whose code becomes the exit code.  must: a library call that fails with its message alone.
inline std::string g_tool;
[[noreturn]] inline void die(const std::string &msg, int rc = 1)
{
    fprintf(stderr, "%s%s%s\n", g_tool.c_str(), g_tool.empty() ? "" : ": ", msg.c_str());
    exit(rc);
}
[[noreturn]] inline void fail(const std::string &msg) { die(msg, 2); }
#define CHK(call)                                                                                 \
    do {                                                                                          \
        if (int rc_ = (call)) die(std::string(#call) + ": " + dh_last_error(), rc_ < 0 ? -rc_ : rc_); \
    } while (0)
inline void must(int rc)
{
    if (rc) fail(dh_last_error());
}

// ---------------------------------------------------------------------------------- options
// --key=<value>: `key` is written with its dashes and the '='; the value must not be empty (`--mask=` matches nothing)
inline bool long_value(const std::string &a, const std::string &key, std::string *value = nullptr)
{
    if (a.size() <= key.size() || a.compare(0, key.size(), key) != 0) return false;
    if (value) *value = a.substr(key.size());
    return true;
}
// -X<value>, attached and not empty (-T8, -mdust); one dash only: --m... is never the short form of -m
inline bool short_value(const std::string &a, char letter, std::string *value = nullptr)
{
    if (a.size() <= 2 || a[0] != '-' || a[1] != letter) return false;
    if (value) *value = a.substr(2);
    return true;
}
inline bool is_option(const std::string &a) { return a.size() > 1 && a[0] == '-'; }

// The lenient numbers (chain-local-alignments, validate-regions, collect): an empty value keeps the default, a value that is
// not consumed to its end exits 2.
inline void lenient_number(const std::string &v, int32_t *out)
{
    if (v.empty()) return;
    char *end = nullptr;
    *out = (int32_t)strtol(v.c_str(), &end, 10);
    if (*end) fail("an option's value is not a number");
}
inline void lenient_number(const std::string &v, double *out)
{
    if (v.empty()) return;
    char *end = nullptr;
    *out = strtod(v.c_str(), &end);
    if (*end) fail("an option's value is not a number");
}
// The strict numbers (mask-repetitive-regions, filter-mask, check-results): `a` is --key=<0 .. INT32_MAX>; an empty value
// or anything else prints the usage and exits 1.  False when `a` is another option.
inline bool strict_number(const std::string &a, const std::string &key, long long *out, const std::string &usage)
{
    if (a.compare(0, key.size(), key) != 0) return false;
    const char *v = a.c_str() + key.size();
    char *end = nullptr;
    *out = strtoll(v, &end, 10);
    if (end == v || *end || *out < 0 || *out > INT32_MAX) die("unknown or malformed option " + a + "\n" + usage);
    return true;
}

// the options DENTIST passes to every sub-command and that mean nothing here
inline bool ignored_option(const std::string &a)
{
    return a == "-v" || a == "--quiet" || long_value(a, "--config=") || short_value(a, 'T') || long_value(a, "--threads=");
}
inline void notice_ignored(const char *which = "--config, -v, --quiet, -T and --threads")
{
    fprintf(stderr, "%s: %s have no effect here\n", g_tool.c_str(), which);
}

// ---------------------------------------------------------------------------------- handles
// Every object of the library a tool owns, destroyed with its scope (in reverse order of declaration: the context is
// declared before what is created from it).  into(h) is the `T **` of a creating call; h owns the object after the call.
template <class T, void (*Destroy)(T *)>
struct Destroyer {
    void operator()(T *p) const { Destroy(p); }
};
template <class T, void (*Destroy)(T *)>
using Handle = std::unique_ptr<T, Destroyer<T, Destroy>>;
using Ctx = Handle<dh_ctx, dh_ctx_destroy>;
using Dazz = Handle<dh_dazz, dh_dazz_close>;
using Db = Handle<dh_db, dh_db_destroy>;
using LaSet = Handle<dh_la_set, dh_la_set_destroy>;
using EditPaths = Handle<dh_edit_paths, dh_edit_paths_destroy>;
using ExactHits = Handle<dh_exact_hits, dh_exact_hits_destroy>;
using LaChains = Handle<dh_la_chains, dh_la_chains_destroy>;
using MaskResult = Handle<dh_mask_result, dh_mask_result_destroy>;
using RegionResult = Handle<dh_region_result, dh_region_result_destroy>;
using RepeatResult = Handle<dh_repeat_result, dh_repeat_result_destroy>;
using MaskSet = Handle<dh_mask_set, dh_mask_set_destroy>;
using GapReport = Handle<dh_gap_report, dh_gap_report_destroy>;
using Scaffold = Handle<dh_scaffold, dh_scaffold_destroy>;
using Pileups = Handle<dh_pileups, dh_pileups_destroy>;

template <class H>
struct Into {
    H &h;
    typename H::pointer p = nullptr;
    ~Into() { h.reset(p); }
    operator typename H::pointer *() { return &p; }
};
template <class H>
Into<H> into(H &h)
{
    return Into<H>{h};
}

inline Dazz open_dazz(const std::string &path)
{
    dh_dazz *d = nullptr;
    CHK(dh_dazz_open(path.c_str(), &d));
    return Dazz(d);
}
inline LaSet read_las(const std::string &path)
{
    dh_la_set *set = nullptr;
    CHK(dh_las_read(path.c_str(), &set));
    return LaSet(set);
}

// a DAZZ_DB on the device: with a context of its own, or as another DB on the context of the first
struct Dev {
    Ctx own;
    dh_ctx *ctx = nullptr;
    Dazz dz;
    Db db;
    explicit Dev(const std::string &path)
    {
        CHK(dh_ctx_create(0, nullptr, into(own)));
        open(own.get(), path);
    }
    Dev(dh_ctx *shared, const std::string &path) { open(shared, path); }

private:
    void open(dh_ctx *c, const std::string &path)
    {
        ctx = c;
        dz = open_dazz(path);
        CHK(dh_db_create(ctx, dh_dazz_bases(dz.get()), dh_dazz_offsets(dz.get()), dh_dazz_nreads(dz.get()), nullptr, into(db)));
    }
};

// ---------------------------------------------------------------------------------- masks
// Mask track `name` of the opened DB: ptr has a slot per read and one more, iv is never an empty array.  "" or what failed.
inline std::string read_mask(const dh_dazz *da, const std::string &db_path, const std::string &name, std::vector<int64_t> &ptr,
                             std::vector<int32_t> &iv)
{
    ptr.assign((size_t)dh_dazz_nreads(da) + 1, 0);
    const int64_t cnt = dh_dazz_read_mask(da, db_path.c_str(), name.c_str(), ptr.data(), nullptr, 0);
    if (cnt < 0) return "mask " + name + ": " + dh_last_error();
    iv.assign((size_t)(2 * cnt) + 2, 0);
    if (dh_dazz_read_mask(da, db_path.c_str(), name.c_str(), ptr.data(), iv.data(), cnt) < 0) return "mask " + name + ": " + dh_last_error();
    return "";
}

// The int64 track extra `name` of mask `mask`: false when the mask has no extra of that name, exit 2 on anything else.
inline bool read_extra(const std::string &db_path, const std::string &mask, const char *name, std::vector<int64_t> &data)
{
    int32_t vtype = DH_EXTRA_INT64;
    const int64_t cnt = dh_dazz_read_extra(db_path.c_str(), mask.c_str(), name, &vtype, nullptr, nullptr, 0);
    if (cnt == DH_ENOTFOUND) return false;
    if (cnt < 0) fail("mask " + mask + ": " + dh_last_error());
    data.assign((size_t)cnt + 1, 0);  // (never an empty array)
    if (dh_dazz_read_extra(db_path.c_str(), mask.c_str(), name, &vtype, nullptr, data.data(), cnt) != cnt) fail("mask " + mask + ": " + dh_last_error());
    data.resize((size_t)cnt);
    return true;
}

// the intervals of every contig sorted, intersecting or touching ones merged (iv may come out empty: the caller that hands
// it to the library appends an element)
inline void merge_intervals(std::vector<std::vector<std::pair<int32_t, int32_t>>> &per, std::vector<int64_t> &ptr, std::vector<int32_t> &iv)
{
    ptr.assign(1, 0);
    iv.clear();
    for (auto &v : per) {
        std::sort(v.begin(), v.end());
        const size_t first = iv.size();
        for (const auto &x : v) {
            if (iv.size() > first && x.first <= iv.back())
                iv.back() = std::max(iv.back(), x.second);
            else {
                iv.push_back(x.first);
                iv.push_back(x.second);
            }
        }
        ptr.push_back((int64_t)iv.size() / 2);
    }
}

// dh_dazz_write_mask of a result: a result without intervals may have no array at all
inline int write_mask(const std::string &db_path, const std::string &name, int32_t n, const int64_t *ptr, const int32_t *iv, int64_t count)
{
    static const int32_t no_iv[2] = {0, 0};
    return dh_dazz_write_mask(db_path.c_str(), name.c_str(), n, ptr, count > 0 ? iv : no_iv);
}

// ---------------------------------------------------------------------------------- records, gaps
// the records of a .las with the ids of the file (trimmed DB ids) shifted to those of the opened views
inline std::vector<dh_la> shifted_records(const dh_la_set *set, int32_t first_a, int32_t first_b)
{
    std::vector<dh_la> las(dh_la_set_records(set), dh_la_set_records(set) + dh_la_set_count(set));
    for (dh_la &l : las) {
        l.aread -= first_a;
        l.bread -= first_b;
    }
    return las;
}

// contigs c and c + 1 follow each other in one scaffold of the .dam: a gap of the assembly (getScaffoldStructure)
inline bool scaffold_neighbours(const dh_dazz *dz, int32_t c)
{
    return dh_dazz_origin(dz)[c + 1] > dh_dazz_origin(dz)[c] && strcmp(dh_dazz_header(dz, c), dh_dazz_header(dz, c + 1)) == 0;
}
