// ps_outfiles.h -- how every mode publishes its output files, and the three file helpers the modes share.  Host only.
// The entry function of a mode owns one OutFiles: it declares every output, hands the writers the temporary paths, renames when a
// step (or the whole call) is done and says keep().  A call that ends any other way leaves no temporary and no file it published.
#pragma once
#include <sys/stat.h>
#include <unistd.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "ps_error.h"

namespace ps {

inline bool same_file(const char *a, const char *b)    // the same path, or two paths to one file (device and inode)
{
    if (!std::strcmp(a, b)) return true;
    struct stat sa, sb;
    return stat(a, &sa) == 0 && stat(b, &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}
// text -> file, checked.  Nothing is removed: a file that was not written whole is its owner's (OutFiles) to clean up
inline void write_text_file(const std::string &path, const std::string &text)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    const bool ok = f && std::fwrite(text.data(), 1, text.size(), f) == text.size();
    if (!f || std::fclose(f) != 0 || !ok) throw Error("cannot write " + path);
}
inline std::string read_whole_file(const char *path)  // file -> text, checked; one allocation for a regular file
{
    FILE *f = std::fopen(path, "rb");
    if (!f) throw Error(std::string("cannot open ") + path);
    struct Closer { FILE *f; ~Closer() { std::fclose(f); } } closer{f};
    std::string out; struct stat sb;
    if (fstat(fileno(f), &sb) == 0 && S_ISREG(sb.st_mode)) out.reserve((size_t)sb.st_size);
    std::vector<char> chunk((size_t)1 << 20); size_t got;
    while ((got = std::fread(chunk.data(), 1, chunk.size(), f)) > 0) out.append(chunk.data(), got);
    if (std::ferror(f)) throw Error(std::string("cannot read ") + path);
    return out;
}

class OutFiles {
    struct File { std::string name, tmp; bool published; };
    const std::string suffix; std::vector<File> files; bool kept = false;
    File &find(const std::string &name) { for (File &f : files) if (f.name == name) return f; throw Error("internal: " + name + " was not declared as an output"); }
    void rename_one(File &f)
    {
        if (f.published || std::rename(f.tmp.c_str(), f.name.c_str()) != 0) throw Error("cannot rename " + f.tmp + " to " + f.name);
        f.published = true;
    }
public:
    explicit OutFiles(const char *tmp_suffix) : suffix(tmp_suffix) {}
    OutFiles(const OutFiles &) = delete;
    // without keep(): every temporary that is still there and every file this object has published go (unlink: never a directory),
    // and nothing else -- a final name the call did not reach keeps what it held
    ~OutFiles() { if (!kept) for (const File &f : files) ::unlink((f.published ? f.name : f.tmp).c_str()); }
    // declares an output and returns the temporary path to write it to; the second form for a writer that derives the path itself
    std::string add(const std::string &name) { return add(name, name + suffix); }
    std::string add(const std::string &name, const std::string &tmp) { files.push_back(File{name, tmp, false}); return tmp; }
    const std::string &tmp(const std::string &name) { return find(name).tmp; }
    std::vector<std::string> paths() const { std::vector<std::string> all; for (const File &f : files) { all.push_back(f.name); all.push_back(f.tmp); } return all; }   // every path the call may touch
    // inputs: the files the call reads (null and "" are skipped); asked before anything is written.  The message: who "the output"
    // <path> how <input>.  A refused set forgets its names: the temporary it would clean up may be the input itself
    void refuse_inputs(const std::vector<const char *> &inputs, const std::string &who, const char *how = " would overwrite the input ")
    {
        for (const std::string &p : paths()) for (const char *in : inputs)
            if (in && in[0] && same_file(p.c_str(), in)) { files.clear(); throw Error(who + "the output " + p + how + in); }
    }
    void publish(const std::string &name) { rename_one(find(name)); }
    // the rest, in the order declared.  Several renames are not one: the failure that can be seen coming, a final name taken by a
    // directory, is looked for before the first, so that it replaces no file
    void publish_all()
    {
        struct stat sb;
        for (const File &f : files) if (!f.published && stat(f.name.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode)) throw Error("cannot rename " + f.tmp + " to " + f.name + ": a directory");
        for (File &f : files) if (!f.published) rename_one(f);
    }
    void keep() { kept = true; }                           // the call has succeeded
};

}  // namespace ps
