// outfiles_check.cpp -- drives csrc/ps_outfiles.h alone (tests/test_outfiles_cpu.py): a call's output files from their declaration
// to keep() or to the clean-up of a call that failed, the input-overwrite check and the three file helpers, in a directory of its own.
// A plain program: every check that fails prints what it expected and ends the run with status 1.
#include <cstdlib>
#include <dirent.h>
#include <map>
#include "ps_outfiles.h"

using namespace ps;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// the directory as name -> bytes ("<dir>" for a directory)
static std::map<std::string, std::string> listing(const std::string &dir)
{
    std::map<std::string, std::string> out;
    DIR *d = ::opendir(dir.c_str());
    CHECK(d);
    while (const dirent *e = ::readdir(d)) {
        const std::string n = e->d_name, p = dir + "/" + n;
        if (n == "." || n == "..") continue;
        struct stat sb;
        CHECK(::lstat(p.c_str(), &sb) == 0);
        out[n] = S_ISDIR(sb.st_mode) ? "<dir>" : read_whole_file(p.c_str());
    }
    ::closedir(d);
    return out;
}
template <class F> static std::string error_of(F f) { try { f(); } catch (const Error &e) { return e.what(); } return ""; }
static bool has(const std::string &s, const std::string &part) { return s.find(part) != std::string::npos; }

static void success(const std::string &dir)
{
    const auto before = listing(dir);
    {
        OutFiles files(".t-tmp");
        const std::string a = files.add(dir + "/a"), b = files.add(dir + "/b"), c = files.add(dir + "/c", dir + "/elsewhere.c");
        CHECK(a == dir + "/a.t-tmp" && b == dir + "/b.t-tmp" && c == dir + "/elsewhere.c" && files.tmp(dir + "/b") == b);
        write_text_file(a, "first"); write_text_file(b, std::string("se\0cond\n", 8)); write_text_file(c, "");
        CHECK(listing(dir).size() == before.size() + 3 && !listing(dir).count("a"));      // nothing under a final name yet
        files.publish(dir + "/b");                                                         // a step of its own, then the rest in order
        CHECK(listing(dir).count("b") && !listing(dir).count("b.t-tmp") && !listing(dir).count("a"));
        files.publish_all();
        CHECK(has(error_of([&] { files.publish(dir + "/b"); }), "cannot rename"));      // not twice
        CHECK(has(error_of([&] { files.publish(dir + "/never"); }), "was not declared"));
        files.keep();
    }
    auto want = before;
    want["a"] = "first"; want["b"] = std::string("se\0cond\n", 8); want["c"] = "";
    CHECK(listing(dir) == want);
    {                                                                                      // again over the files of the first call: replaced whole
        OutFiles files(".t-tmp");
        write_text_file(files.add(dir + "/a"), "1"); write_text_file(files.add(dir + "/b"), "2");
        files.publish_all(); files.keep();
    }
    want["a"] = "1"; want["b"] = "2";
    CHECK(listing(dir) == want);
    std::printf("ok success\n");
}

static void no_keep(const std::string &dir)
{
    write_text_file(dir + "/old", "from before");
    const auto before = listing(dir);
    for (int n_published = 0; n_published <= 3; ++n_published) {
        {
            OutFiles files(".t-tmp");
            const char *names[3] = {"/x", "/y", "/z"};
            for (const char *n : names) write_text_file(files.add(dir + n), n);
            files.add(dir + "/declared-only");                                             // its writer was never reached
            for (int k = 0; k < n_published; ++k) files.publish(dir + names[k]);
            CHECK((int)listing(dir).size() == (int)before.size() + 3);
        }
        CHECK(listing(dir) == before);
    }
    try { OutFiles files(".t-tmp"); write_text_file(files.add(dir + "/x"), "x"); throw Error("the call failed"); } catch (const Error &) {}
    CHECK(listing(dir) == before);
    std::printf("ok no_keep\n");
}

static void rename_fails(const std::string &dir)
{
    CHECK(::mkdir((dir + "/b").c_str(), 0755) == 0);
    write_text_file(dir + "/b/inside", "kept");
    const auto before = listing(dir);
    // step by step: the first rename is done when the second fails
    std::string err = error_of([&] {
        OutFiles files(".t-tmp");
        for (const char *n : {"/a", "/b", "/c"}) write_text_file(files.add(dir + n), n);
        files.publish(dir + "/a");
        CHECK(listing(dir).count("a"));
        files.publish(dir + "/b");
    });
    CHECK(has(err, "cannot rename " + dir + "/b.t-tmp to " + dir + "/b") && listing(dir) == before);
    // all together: a name taken by a directory is seen before the first rename
    err = error_of([&] {
        OutFiles files(".t-tmp");
        for (const char *n : {"/a", "/b", "/c"}) write_text_file(files.add(dir + n), n);
        files.publish_all();
    });
    CHECK(has(err, "cannot rename " + dir + "/b.t-tmp to " + dir + "/b") && listing(dir) == before);
    // all together, and the failure no look ahead finds: a temporary that is gone
    err = error_of([&] {
        OutFiles files(".t-tmp");
        for (const char *n : {"/a", "/lost", "/c"}) write_text_file(files.add(dir + n), n);
        CHECK(::unlink((dir + "/lost.t-tmp").c_str()) == 0);
        try { files.publish_all(); } catch (...) { CHECK(listing(dir).count("a") && listing(dir).count("c.t-tmp")); throw; }
    });
    CHECK(has(err, "cannot rename " + dir + "/lost.t-tmp") && listing(dir) == before);
    CHECK(read_whole_file((dir + "/b/inside").c_str()) == "kept");
    std::printf("ok rename_fails\n");
}

static void preexisting(const std::string &dir)
{
    write_text_file(dir + "/a", "old a"); write_text_file(dir + "/b", "old b");
    CHECK(::mkdir((dir + "/c").c_str(), 0755) == 0);
    const auto before = listing(dir);
    {                                                                                      // fails before any output is published
        OutFiles files(".t-tmp");
        write_text_file(files.add(dir + "/a"), "new a"); files.add(dir + "/b");
    }
    CHECK(listing(dir) == before);
    const std::string err = error_of([&] {                                                 // fails where its outputs are published together
        OutFiles files(".t-tmp");
        for (const char *n : {"/a", "/b", "/c"}) write_text_file(files.add(dir + n), "new");
        files.publish_all(); files.keep();
    });
    CHECK(!err.empty() && listing(dir) == before);
    {                                                                                      // one that WAS replaced goes with the failed call; the other stays
        OutFiles files(".t-tmp");
        write_text_file(files.add(dir + "/a"), "new a"); write_text_file(files.add(dir + "/b"), "new b");
        files.publish(dir + "/a");
    }
    auto want = before; want.erase("a");
    CHECK(listing(dir) == want);
    std::printf("ok preexisting\n");
}

static void unopenable(const std::string &dir)
{
    const auto before = listing(dir);
    const std::string err = error_of([&] {
        OutFiles files(".t-tmp");
        write_text_file(files.add(dir + "/here"), "x");
        write_text_file(files.add(dir + "/no/such/dir/out"), "y");
    });
    CHECK(err == "cannot write " + dir + "/no/such/dir/out.t-tmp" && listing(dir) == before);
    std::printf("ok unopenable\n");
}

static void paths(const std::string &dir)
{
    OutFiles files(".t-tmp");
    CHECK(files.paths().empty());
    files.add("a"); files.add(dir + "/b.bam"); files.add(dir + "/b.bam.bai", dir + "/b.bam.t-tmp.bai");
    const std::vector<std::string> want = {"a", "a.t-tmp", dir + "/b.bam", dir + "/b.bam.t-tmp", dir + "/b.bam.bai", dir + "/b.bam.t-tmp.bai"};
    CHECK(files.paths() == want);
    files.keep();
    std::printf("ok paths\n");
}

static void refuse_inputs(const std::string &dir)
{
    const std::string in = dir + "/in.txt";
    write_text_file(in, "input");
    CHECK(::mkdir((dir + "/sub").c_str(), 0755) == 0);
    CHECK(::link(in.c_str(), (dir + "/hard").c_str()) == 0 && ::symlink("in.txt", (dir + "/soft").c_str()) == 0);
    CHECK(::link(in.c_str(), (dir + "/o4.t-tmp").c_str()) == 0 && ::link(in.c_str(), (dir + "/o5.elsewhere").c_str()) == 0);
    const auto before = listing(dir);
    struct Case { std::string out, named; };
    const Case cases[] = {{in, in}, {dir + "/sub/../in.txt", dir + "/sub/../in.txt"}, {dir + "/hard", dir + "/hard"}, {dir + "/soft", dir + "/soft"},
                          {dir + "/o4", dir + "/o4.t-tmp"}};                               // the last: the input is what the output's temporary name names
    for (const Case &c : cases) {
        OutFiles files(".t-tmp");
        files.add(dir + "/fine"); files.add(c.out);
        const std::string err = error_of([&] { files.refuse_inputs({nullptr, "", (dir + "/other").c_str(), in.c_str()}, "mode: "); });
        CHECK(err == "mode: the output " + c.named + " would overwrite the input " + in);
    }
    {
        OutFiles files(".t-tmp");
        files.add(dir + "/o5", dir + "/o5.elsewhere");                                     // the explicit temporary
        CHECK(error_of([&] { files.refuse_inputs({in.c_str()}, "mode: ", " may not be the input file "); }) == "mode: the output " + dir + "/o5.elsewhere may not be the input file " + in);
    }
    {
        OutFiles files(".t-tmp");
        files.add(dir + "/fine"); files.add(in + ".more"); files.add(dir + "/missing/out");
        files.refuse_inputs({in.c_str(), nullptr, "", (dir + "/absent").c_str()}, "mode: ");        // nothing to refuse
        files.refuse_inputs({}, "mode: ");
    }
    CHECK(listing(dir) == before);                                                         // a refusal removes nothing: the input's other names stand
    std::printf("ok refuse_inputs\n");
}

static void text_file(const std::string &dir)
{
    write_text_file(dir + "/t", "one");
    write_text_file(dir + "/t", std::string("t\0wo", 4));
    CHECK(read_whole_file((dir + "/t").c_str()) == std::string("t\0wo", 4));
    std::string big((size_t)3 << 20, 'x'); big[12345] = '\n';
    write_text_file(dir + "/big", big);
    CHECK(read_whole_file((dir + "/big").c_str()) == big);
    CHECK(::mkdir((dir + "/d").c_str(), 0755) == 0);
    write_text_file(dir + "/d/inside", "kept");
    const auto before = listing(dir);
    CHECK(error_of([&] { write_text_file(dir + "/d", "x"); }) == "cannot write " + dir + "/d");            // a directory: still there, with what it holds
    CHECK(error_of([&] { write_text_file(dir + "/none/f", "x"); }) == "cannot write " + dir + "/none/f");
    CHECK(listing(dir) == before && read_whole_file((dir + "/d/inside").c_str()) == "kept");
    CHECK(error_of([&] { read_whole_file((dir + "/absent").c_str()); }) == "cannot open " + dir + "/absent");
    CHECK(has(error_of([&] { read_whole_file((dir + "/d").c_str()); }), "cannot read " + dir + "/d"));
    CHECK(same_file((dir + "/t").c_str(), (dir + "/d/../t").c_str()) && !same_file((dir + "/t").c_str(), (dir + "/big").c_str()));
    CHECK(same_file((dir + "/absent").c_str(), (dir + "/absent").c_str()) && !same_file((dir + "/absent").c_str(), (dir + "/absent2").c_str()));
    std::printf("ok text_file\n");
}

int main(int argc, char **argv)
{
    const std::string what = argc > 1 ? argv[1] : "", dir = argc > 2 ? argv[2] : "";
    if (dir.empty()) { std::printf("usage: outfiles_check success|no_keep|rename_fails|preexisting|unopenable|paths|refuse_inputs|text_file DIR\n"); return 2; }
    if (what == "success") success(dir);
    else if (what == "no_keep") no_keep(dir);
    else if (what == "rename_fails") rename_fails(dir);
    else if (what == "preexisting") preexisting(dir);
    else if (what == "unopenable") unopenable(dir);
    else if (what == "paths") paths(dir);
    else if (what == "refuse_inputs") refuse_inputs(dir);
    else if (what == "text_file") text_file(dir);
    else return 2;
    return 0;
}
