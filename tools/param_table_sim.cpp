// The model table (border_amd/csrc/param_table.hpp) on a CPU: a fake agent whose "device" arenas are host vectors and whose
// checkpoint files are in-memory buffers runs one fixed scenario and prints what happened; tests/test_param_table_host.py builds
// this with -fsanitize=address,undefined, runs it and compares the output with its own restatement of the rules.
//
// Models: 0 `net`  reference [3][5] <-> arena [8][4] (transposed, both dimensions padded)       15 values in 32 floats
//         1 `q`    7 values at the start of 8 floats                                          (another size, plain layout)
//         2 `temp` one value in 4 floats
//         3 `q_tgt` as 1
// Files:  "net" = models 0 and 2 concatenated;  "q" = model 1;  "q.tgt" = saved from model 3, loaded into model 1.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../border_amd/csrc/param_table.hpp"

using namespace bdr;

struct Fake : ParamTable {
    std::vector<float> mem[4] = {std::vector<float>(32), std::vector<float>(8), std::vector<float>(4), std::vector<float>(8)};
    std::map<std::string, std::vector<float>> disk;
    std::string corrupt;                  // stem whose read fails
    std::vector<std::string> trace;

    bool param_view(int which, ParamView* v) override
    {
        if (which < 0 || which > 3) return false;
        if (which == 0)
            *v = {mem[0].data(), 32, 15, [](const float* a, float* r) { for (int o = 0; o < 3; ++o) for (int k = 0; k < 5; ++k) r[o * 5 + k] = a[k * 4 + o]; },
                  [](const float* r, float* a) { for (int o = 0; o < 3; ++o) for (int k = 0; k < 5; ++k) a[k * 4 + o] = r[o * 5 + k]; }};
        else if (which == 2)
            *v = {mem[2].data(), 4, 1, [](const float* a, float* r) { r[0] = a[0]; }, [](const float* r, float* a) { a[0] = r[0]; }};
        else
            *v = {mem[which].data(), 8, 7, [](const float* a, float* r) { for (int i = 0; i < 7; ++i) r[i] = a[i]; },
                  [](const float* r, float* a) { for (int i = 0; i < 7; ++i) a[i] = r[i]; }};
        return true;
    }
    void checkpoint_files(std::vector<CheckpointFile>& files) override
    {
        files = {{"net", {{"w", {3, 5}}, {"temp", {1}}}, {0, 2}, {0, 2}}, {"q", {{"q", {7}}}, {1}, {1}}, {"q.tgt", {{"q", {7}}}, {3}, {1}}};
    }
    int32_t params_quiesce() override { trace.push_back("quiesce"); return 0; }
    int32_t params_written(int which) override { trace.push_back("written:" + std::to_string(which)); return 0; }
    void arena_handed_out(int which) override { trace.push_back("handed_out:" + std::to_string(which)); }
    int model_of(const float* arena) const { for (int i = 0; i < 4; ++i) if (arena == mem[i].data()) return i; return -1; }
    int32_t arena_to_host(const float* arena, float* host, size_t n) override
    {
        trace.push_back("to_host:" + std::to_string(model_of(arena)));
        for (size_t i = 0; i < n; ++i) host[i] = arena[i];
        return 0;
    }
    int32_t arena_from_host(float* arena, const float* host, size_t n) override
    {
        trace.push_back("from_host:" + std::to_string(model_of(arena)));
        for (size_t i = 0; i < n; ++i) arena[i] = host[i];
        return 0;
    }
    int32_t file_write(const CheckpointFile& f, const char*, const float* data, size_t n) override
    {
        trace.push_back("write:" + f.stem);
        disk[f.stem].assign(data, data + n);
        return 0;
    }
    int32_t file_read(const CheckpointFile& f, const char*, float* data, size_t n) override
    {
        trace.push_back("read:" + f.stem);
        size_t want = 0;
        for (const auto& t : f.tensors) { size_t k = 1; for (auto d : t.dims) k *= d; want += k; }
        if (f.stem == corrupt || !disk.count(f.stem) || disk[f.stem].size() != n || want != n) return 7;
        for (size_t i = 0; i < n; ++i) data[i] = disk[f.stem][i];
        return 0;
    }
    int32_t param_error(const std::string& what) override { printf("error %s\n", what.c_str()); return 3; }

    void show_trace(const char* op)
    {
        printf("trace %s:", op);
        for (const auto& t : trace) printf(" %s", t.c_str());
        printf("\n");
        trace.clear();
    }
    void show_arenas()
    {
        for (int i = 0; i < 4; ++i) { printf("arena %d:", i); for (float x : mem[i]) printf(" %g", x); printf("\n"); }
    }
};

static std::vector<float> values(int which, size_t n, int generation)
{
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (float)(generation * 10000 + which * 100 + (int)i) + 0.5f;
    return v;
}

int main()
{
    Fake a;
    for (auto& m : a.mem) for (auto& x : m) x = -1.f;      // stale padding: a set must clear it
    for (int which : {-1, 0, 1, 2, 3, 4, 100}) printf("count %d %llu\n", which, (unsigned long long)a.param_count(which));
    a.trace.clear();
    // set then get, every view
    for (int which = 0; which < 4; ++which) {
        const auto v = values(which, a.param_count(which), 1);
        a.trace.clear();
        printf("set %d -> %d\n", which, a.set_params(which, v.data(), v.size()));
        a.show_trace("set_params");
        std::vector<float> back(v.size(), 0.f);
        printf("get %d -> %d:", which, a.get_params(which, back.data(), back.size()));
        for (float x : back) printf(" %g", x);
        printf("\n");
        a.show_trace("get_params");
    }
    a.show_arenas();
    // refused calls change nothing
    {
        std::vector<float> v(64, 9.f);
        printf("set unknown -> %d\n", a.set_params(4, v.data(), 15));
        printf("get unknown -> %d\n", a.get_params(-1, v.data(), 15));
        printf("set short -> %d\n", a.set_params(0, v.data(), 14));
        printf("get long -> %d\n", a.get_params(1, v.data(), 8));
        size_t n = 99;
        const float* p = a.arena(7, &n);
        printf("arena unknown -> %s %zu\n", p ? "ptr" : "null", n);
        a.show_trace("refused");
        a.show_arenas();
    }
    {
        size_t n = 0;
        float* p = a.arena(1, &n);
        printf("arena 1 -> model %d %zu\n", a.model_of(p), n);
        a.show_trace("arena");
    }
    printf("save -> %d\n", a.save("dir"));
    a.show_trace("save");
    for (const auto& f : a.disk) { printf("file %s:", f.first.c_str()); for (float x : f.second) printf(" %g", x); printf("\n"); }
    // other values everywhere, then a load whose LAST file is corrupt: nothing may change
    for (int which = 0; which < 4; ++which) { const auto v = values(which, a.param_count(which), 2); (void)a.set_params(which, v.data(), v.size()); }
    a.trace.clear();
    a.corrupt = "q.tgt";
    printf("load corrupt -> %d\n", a.load("dir"));
    a.show_trace("load");
    a.show_arenas();
    a.corrupt.clear();
    printf("load -> %d\n", a.load("dir"));
    a.show_trace("load");
    a.show_arenas();
    return 0;
}
