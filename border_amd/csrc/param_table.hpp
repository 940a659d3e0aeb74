// The model table: what every agent handle answers about its parameters - how many reference-layout values model `which` has, give
// me them, take them, hand me the raw arena, save / load your checkpoint files - written once over a few questions an agent answers
// (param_view, checkpoint_files and three hooks).  No HIP here: copies between an arena and the host and the checkpoint containers
// are reached through virtuals (bdr_agent, agent_base.hpp, supplies them), so tools/param_table_sim.cpp runs this logic on a CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace bdr {

// named f32 tensor of a checkpoint container (reference variable names)
struct NamedTensor { std::string name; std::vector<uint64_t> dims; };

// One (model, role): the device arena in the kernels' layout and its reference-layout vector
struct ParamView {
    float* arena = nullptr;        // device
    size_t arena_floats = 0;
    uint64_t count = 0;            // reference-layout elements
    std::function<void(const float* arena_copy, float* ref)> to_reference;
    std::function<void(const float* ref, float* arena_copy)> from_reference;   // arena_copy is all zero on entry: padding stays 0
};

// One checkpoint file: on save the reference vectors of `save_from` are concatenated into it, on load it is split over `load_into`
struct CheckpointFile {
    std::string stem;
    std::vector<NamedTensor> tensors;
    std::vector<int> save_from, load_into;
};

struct ParamTable {
    virtual ~ParamTable() = default;
    // ---- what an agent supplies ----
    virtual bool param_view(int which, ParamView* v) = 0;                      // false: unknown id.  The only place that knows the numbering
    virtual void checkpoint_files(std::vector<CheckpointFile>& files) = 0;     // in save / load order
    virtual int32_t params_quiesce() { return 0; }                             // first in every entry point below that touches an arena
    virtual int32_t params_written(int /*which*/) { return 0; }                // after an arena was written from a reference vector
    virtual void arena_handed_out(int /*which*/) {}                            // from arena()
    // ---- what the handle supplies: the copies, the containers, the error channel ----
    virtual int32_t arena_to_host(const float* arena, float* host, size_t n) = 0;
    virtual int32_t arena_from_host(float* arena, const float* host, size_t n) = 0;
    virtual int32_t file_write(const CheckpointFile& f, const char* dir, const float* data, size_t n) = 0;
    virtual int32_t file_read(const CheckpointFile& f, const char* dir, float* data, size_t n) = 0;
    virtual int32_t param_error(const std::string& what) = 0;

    // ---- the six entry points ----
    // reads no arena, so nothing is quiesced: it launches nothing and needs no current device
    uint64_t param_count(int which)
    {
        ParamView v;
        return param_view(which, &v) ? v.count : 0;
    }
    int32_t get_params(int which, float* out, uint64_t n)
    {
        if (const int32_t st = params_quiesce()) return st;
        return read_view(which, out, n);
    }
    int32_t set_params(int which, const float* in, uint64_t n)
    {
        if (const int32_t st = params_quiesce()) return st;
        return write_view(which, in, n);
    }
    float* arena(int which, size_t* n)
    {
        (void)params_quiesce();
        ParamView v;
        const bool known = param_view(which, &v);
        if (n) *n = known ? v.arena_floats : 0;
        if (!known) return nullptr;
        arena_handed_out(which);
        return v.arena;
    }
    int32_t save(const char* dir)
    {
        if (const int32_t st = params_quiesce()) return st;
        std::vector<CheckpointFile> files;
        checkpoint_files(files);
        for (const auto& f : files) {
            std::vector<float> data(total(f.save_from));
            size_t o = 0;
            for (int id : f.save_from) {
                const uint64_t n = param_count(id);
                if (const int32_t st = read_view(id, data.data() + o, n)) return st;
                o += n;
            }
            if (const int32_t st = file_write(f, dir, data.data(), data.size())) return st;
        }
        return 0;
    }
    // every file is read and validated before any arena is written: a failed load leaves the agent as it was.  Then the files are
    // applied in their order (a later file wins where two are loaded into the same model)
    int32_t load(const char* dir)
    {
        if (const int32_t st = params_quiesce()) return st;
        std::vector<CheckpointFile> files;
        checkpoint_files(files);
        std::vector<std::vector<float>> data(files.size());
        for (size_t i = 0; i < files.size(); ++i) {
            data[i].resize(total(files[i].load_into));
            if (const int32_t st = file_read(files[i], dir, data[i].data(), data[i].size())) return st;
        }
        for (size_t i = 0; i < files.size(); ++i) {
            size_t o = 0;
            for (int id : files[i].load_into) {
                const uint64_t n = param_count(id);
                if (const int32_t st = write_view(id, data[i].data() + o, n)) return st;
                o += n;
            }
        }
        return 0;
    }
    // the tensors of checkpoint file i (param_stats of a model names its variables as its file does)
    std::vector<NamedTensor> file_tensors(size_t i)
    {
        std::vector<CheckpointFile> files;
        checkpoint_files(files);
        return files.at(i).tensors;
    }

private:
    size_t total(const std::vector<int>& ids) { size_t n = 0; for (int id : ids) n += param_count(id); return n; }
    int32_t checked_view(int which, uint64_t n, ParamView* v)
    {
        if (!param_view(which, v)) return param_error("unknown model " + std::to_string(which));
        if (n != v->count)
            return param_error("parameter count mismatch: model " + std::to_string(which) + " holds " + std::to_string(v->count) + " values, the caller has " + std::to_string(n));
        return 0;
    }
    int32_t read_view(int which, float* out, uint64_t n)
    {
        ParamView v;
        if (const int32_t st = checked_view(which, n, &v)) return st;
        std::vector<float> host(v.arena_floats);
        if (const int32_t st = arena_to_host(v.arena, host.data(), host.size())) return st;
        v.to_reference(host.data(), out);
        return 0;
    }
    int32_t write_view(int which, const float* in, uint64_t n)
    {
        ParamView v;
        if (const int32_t st = checked_view(which, n, &v)) return st;
        std::vector<float> host(v.arena_floats, 0.f);
        v.from_reference(in, host.data());
        if (const int32_t st = arena_from_host(v.arena, host.data(), host.size())) return st;
        return params_written(which);
    }
};

}  // namespace bdr
