// Observation normaliser of an offline dataset: PenConverter::new / normalize_observation
// (border-minari/src/d4rl/pen/candle.rs:42-74) - per-column mean and std over the dataset, z = (x - mean) / std.
//
// Statistics run on the device in float64 over the f32-rounded elements (pyobj_to_arrayd::<f64, f32>), in a fixed order:
//   k_norm_block   one wave per (block of 64 rows, 64 columns): lane c walks its column twice (mean, then the sum of squared
//                  deviations around that mean) - no cancellation however far a column's mean lies from its spread
//   k_norm_merge   one lane per column folds the blocks into the running (count, mean, M2) in row order (Chan et al.)
//   k_norm_finish  mean -> f32, sqrt(M2 / (n - 1)) -> f32
// so a sequence of accumulate calls gives the same bits on every run.  The rows cross PCIe once, in their own dtype.
#include "common.hpp"

#include <cmath>

using namespace bdr;

constexpr uint64_t NORM_BLOCK_ROWS = 64;            // rows per (mean, M2) block
constexpr uint64_t NORM_STAGE_BYTES = 4ull << 20;   // one staging half (a row of more than 64 KiB raises it to 64 rows)
constexpr uint64_t NORM_MAX_DIM = 1ull << 16;

// partials of block b: part[(b * 2 + 0) * dim + c] = mean, part[(b * 2 + 1) * dim + c] = M2.  Reads: rows [b * 64, min(n, b * 64 + 64))
// x columns < dim of a [n][dim] array; writes: 2 * dim doubles of block b < gridDim.x.
template <typename T>
__global__ __launch_bounds__(64) void k_norm_block(const T* __restrict__ rows, uint64_t n, uint64_t dim, double* __restrict__ part)
{
    const uint64_t c = (uint64_t)blockIdx.y * 64 + threadIdx.x;
    if (c >= dim) return;
    const uint64_t r0 = (uint64_t)blockIdx.x * NORM_BLOCK_ROWS, r1 = min(n, r0 + NORM_BLOCK_ROWS);
    // (a float64 sum of 64 f32 values of equal magnitude is exact: a constant column gives mean == its value and M2 == 0, which finish refuses)
    double sum = 0.0;
    for (uint64_t r = r0; r < r1; ++r) sum += (double)(float)rows[r * dim + c];
    const double mean = sum / (double)(r1 - r0);
    double m2 = 0.0;
    for (uint64_t r = r0; r < r1; ++r) {
        const double d = (double)(float)rows[r * dim + c] - mean;
        m2 += d * d;
    }
    part[((uint64_t)blockIdx.x * 2 + 0) * dim + c] = mean;
    part[((uint64_t)blockIdx.x * 2 + 1) * dim + c] = m2;
}

// running (count0, mean[c], m2[c]) <- merged with the chunk's blocks in order; block b holds min(64, n - 64 b) rows
__global__ __launch_bounds__(64) void k_norm_merge(const double* __restrict__ part, uint64_t n, uint64_t dim, uint64_t count0,
                                                   double* __restrict__ mean, double* __restrict__ m2)
{
    const uint64_t c = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= dim) return;
    double na = (double)count0, ma = count0 ? mean[c] : 0.0, sa = count0 ? m2[c] : 0.0;
    const uint64_t nblocks = (n + NORM_BLOCK_ROWS - 1) / NORM_BLOCK_ROWS;
    for (uint64_t b = 0; b < nblocks; ++b) {
        const double nb = (double)min(NORM_BLOCK_ROWS, n - b * NORM_BLOCK_ROWS);
        const double mb = part[(b * 2 + 0) * dim + c], sb = part[(b * 2 + 1) * dim + c];
        const double nt = na + nb, delta = mb - ma;
        ma += delta * (nb / nt);
        sa += sb + delta * delta * (na * nb / nt);
        na = nt;
    }
    mean[c] = ma; m2[c] = sa;
}

__global__ __launch_bounds__(64) void k_norm_finish(const double* __restrict__ mean, const double* __restrict__ m2, uint64_t dim, uint64_t count,
                                                    float* __restrict__ meanf, float* __restrict__ stdf)
{
    const uint64_t c = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= dim) return;
    meanf[c] = (float)mean[c];
    stdf[c] = (float)sqrt(m2[c] / (double)(count - 1));
}

// out[k][c] = z(rows[k][c]) for k < n, c < dim; row k of the input at rows + k * row_stride bytes, of the output at out + k * out_stride
template <typename T>
__global__ __launch_bounds__(256) void k_norm_apply(const uint8_t* __restrict__ rows, uint64_t row_stride, uint64_t n, uint64_t dim,
                                                    const float* __restrict__ mean, const float* __restrict__ std, uint8_t* __restrict__ out,
                                                    uint64_t out_stride)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * dim) return;
    const uint64_t k = e / dim, c = e % dim;
    const float x = (float)reinterpret_cast<const T*>(rows + k * row_stride)[c];
    reinterpret_cast<float*>(out + k * out_stride)[c] = obs_norm_z(x, mean[c], std[c]);
}

static uint64_t elem_bytes(int32_t dtype) { return dtype == BDR_DTYPE_F64 ? 8 : 4; }

extern "C" {

int32_t bdr_obs_norm_create(int32_t device, uint64_t dim, bdr_obs_norm** out)
{
    BDR_REQUIRE(out, "null argument");
    BDR_REQUIRE(dim >= 1 && dim <= NORM_MAX_DIM, "dim must be in [1, %llu]", (unsigned long long)NORM_MAX_DIM);
    BDR_TRY(ensure_device(device));
    bdr_obs_norm* h = new bdr_obs_norm();
    h->device = device; h->dim = dim;
    h->chunk_rows = std::max<uint64_t>(NORM_BLOCK_ROWS, NORM_STAGE_BYTES / (dim * 8) / NORM_BLOCK_ROWS * NORM_BLOCK_ROWS);
    h->stage_half = h->chunk_rows * dim * 8;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_mean, dim * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_m2, dim * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_meanf, dim * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_stdf, dim * 4);
    if (e != hipSuccess) {
        bdr_obs_norm_destroy(h);
        return fail(BDR_ERR_HIP, "bdr_obs_norm_create: %s", hipGetErrorString(e));
    }
    h->mean.assign(dim, 0.f); h->std.assign(dim, 0.f);
    *out = h;
    return BDR_OK;
}

int32_t bdr_obs_norm_destroy(bdr_obs_norm* h)
{
    if (!h) return BDR_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)hipFree(h->d_mean); (void)hipFree(h->d_m2); (void)hipFree(h->d_part); (void)hipFree(h->d_meanf); (void)hipFree(h->d_stdf);
    (void)hipFree(h->d_raw);
    if (h->stage) (void)hipHostFree(h->stage);
    for (hipEvent_t ev : h->half_free) if (ev) (void)hipEventDestroy(ev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return BDR_OK;
}

// the rows staged in the current half -> device, one k_norm_block / k_norm_merge pair; the other half becomes current
static int32_t norm_flush(bdr_obs_norm* h)
{
    const uint64_t m = h->fill_rows;
    if (m == 0) return BDR_OK;
    const int half = h->half;
    const uint64_t rb = h->dim * elem_bytes(h->fill_dtype);
    uint8_t* st = h->stage + half * h->stage_half;
    uint8_t* dv = h->d_raw + half * h->stage_half;
    BDR_HIP(hipMemcpyAsync(dv, st, m * rb, hipMemcpyHostToDevice, h->stream));
    BDR_HIP(hipEventRecord(h->half_free[half], h->stream));
    const dim3 grid((uint32_t)((m + NORM_BLOCK_ROWS - 1) / NORM_BLOCK_ROWS), (uint32_t)((h->dim + 63) / 64));
    if (h->fill_dtype == BDR_DTYPE_F64) hipLaunchKernelGGL(k_norm_block<double>, grid, dim3(64), 0, h->stream, (const double*)dv, m, h->dim, h->d_part);
    else hipLaunchKernelGGL(k_norm_block<float>, grid, dim3(64), 0, h->stream, (const float*)dv, m, h->dim, h->d_part);
    BDR_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_norm_merge, dim3(grid.y), dim3(64), 0, h->stream, h->d_part, m, h->dim, h->merged, h->d_mean, h->d_m2);
    BDR_HIP(hipGetLastError());
    h->merged += m;
    h->fill_rows = 0;
    h->half ^= 1;
    BDR_HIP(hipEventSynchronize(h->half_free[h->half]));   // the copy out of the half that is filled next (one flush ago) has finished
    return BDR_OK;
}

// Rows are collected in the pinned staging area and go to the device a chunk (chunk_rows, a multiple of 64) at a time, so the
// block boundaries - and with them every bit of the result - depend on the sequence of rows and dtypes alone, not on how the
// caller cut it into calls (an episode per call is the usual cut; a launch per episode would cost more than the arithmetic).
int32_t bdr_obs_norm_accumulate(bdr_obs_norm* h, uint64_t n_rows, const void* rows, int32_t dtype)
{
    BDR_REQUIRE(h, "null normaliser handle");
    BDR_REQUIRE(!h->ready, "bdr_obs_norm_accumulate after finish / set: the statistics are fixed");
    BDR_REQUIRE(dtype == BDR_DTYPE_F32 || dtype == BDR_DTYPE_F64, "dtype must be BDR_DTYPE_F32 or BDR_DTYPE_F64");
    if (n_rows == 0) return BDR_OK;
    BDR_REQUIRE(rows, "null rows");
    BDR_HIP(hipSetDevice(h->device));
    if (!h->stage) {   // staging exists only for handles that compute statistics (not for a converter restored with set)
        BDR_HIP(hipHostMalloc((void**)&h->stage, 2 * h->stage_half, hipHostMallocDefault));
        BDR_HIP(hipMalloc((void**)&h->d_raw, 2 * h->stage_half));
        BDR_HIP(hipMalloc((void**)&h->d_part, h->chunk_rows / NORM_BLOCK_ROWS * 2 * h->dim * 8));
        for (hipEvent_t& ev : h->half_free) BDR_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    if (h->fill_rows && h->fill_dtype != dtype) BDR_TRY(norm_flush(h));
    h->fill_dtype = dtype;
    const uint64_t rb = h->dim * elem_bytes(dtype);
    const uint8_t* src = (const uint8_t*)rows;
    uint64_t done = 0;
    while (done < n_rows) {
        const uint64_t m = std::min(n_rows - done, h->chunk_rows - h->fill_rows);
        memcpy(h->stage + h->half * h->stage_half + h->fill_rows * rb, src + done * rb, m * rb);
        h->fill_rows += m; h->count += m; done += m;
        if (h->fill_rows == h->chunk_rows) BDR_TRY(norm_flush(h));
    }
    return BDR_OK;   // the caller's rows are in the pinned staging area
}

static int32_t check_std(const bdr_obs_norm* h, const float* std, const char* who)
{
    for (uint64_t c = 0; c < h->dim; ++c)
        if (!(std[c] != 0.f) || !std::isfinite(std[c]))
            return fail(BDR_ERR_INVALID, "%s: std of column %llu is %g - a constant or non-finite column cannot be normalised", who,
                        (unsigned long long)c, (double)std[c]);
    return BDR_OK;
}

int32_t bdr_obs_norm_finish(bdr_obs_norm* h)
{
    BDR_REQUIRE(h, "null normaliser handle");
    BDR_REQUIRE(!h->ready, "bdr_obs_norm_finish: the statistics are already fixed");
    BDR_REQUIRE(h->count >= 2, "bdr_obs_norm_finish: %llu rows accumulated, the standard deviation (ddof = 1) needs at least 2",
                (unsigned long long)h->count);
    BDR_HIP(hipSetDevice(h->device));
    BDR_TRY(norm_flush(h));
    hipLaunchKernelGGL(k_norm_finish, dim3((uint32_t)((h->dim + 63) / 64)), dim3(64), 0, h->stream, h->d_mean, h->d_m2, h->dim, h->count, h->d_meanf, h->d_stdf);
    BDR_HIP(hipGetLastError());
    std::vector<float> mean(h->dim), std(h->dim);
    BDR_HIP(hipMemcpyAsync(mean.data(), h->d_meanf, h->dim * 4, hipMemcpyDeviceToHost, h->stream));
    BDR_HIP(hipMemcpyAsync(std.data(), h->d_stdf, h->dim * 4, hipMemcpyDeviceToHost, h->stream));
    BDR_HIP(hipStreamSynchronize(h->stream));
    BDR_TRY(check_std(h, std.data(), "bdr_obs_norm_finish"));
    for (uint64_t c = 0; c < h->dim; ++c)
        if (!std::isfinite(mean[c])) return fail(BDR_ERR_INVALID, "bdr_obs_norm_finish: mean of column %llu is not finite", (unsigned long long)c);
    h->mean.swap(mean); h->std.swap(std);
    h->ready = true;
    return BDR_OK;
}

int32_t bdr_obs_norm_set(bdr_obs_norm* h, const float* mean, const float* std)
{
    BDR_REQUIRE(h && mean && std, "null argument");
    BDR_TRY(check_std(h, std, "bdr_obs_norm_set"));
    BDR_HIP(hipSetDevice(h->device));
    h->mean.assign(mean, mean + h->dim); h->std.assign(std, std + h->dim);
    BDR_HIP(hipMemcpyAsync(h->d_meanf, h->mean.data(), h->dim * 4, hipMemcpyHostToDevice, h->stream));
    BDR_HIP(hipMemcpyAsync(h->d_stdf, h->std.data(), h->dim * 4, hipMemcpyHostToDevice, h->stream));
    BDR_HIP(hipStreamSynchronize(h->stream));
    h->count = 0;
    h->ready = true;
    return BDR_OK;
}

int32_t bdr_obs_norm_get(const bdr_obs_norm* h, float* mean_out, float* std_out, uint64_t* count_out)
{
    BDR_REQUIRE(h, "null normaliser handle");
    BDR_REQUIRE(h->ready, "bdr_obs_norm_get before finish / set: there are no statistics yet");
    if (mean_out) memcpy(mean_out, h->mean.data(), h->dim * 4);
    if (std_out) memcpy(std_out, h->std.data(), h->dim * 4);
    if (count_out) *count_out = h->count;
    return BDR_OK;
}

int32_t bdr_obs_norm_apply(const bdr_obs_norm* h, uint64_t n, const void* rows, int32_t dtype, float* out)
{
    BDR_REQUIRE(h, "null normaliser handle");
    BDR_REQUIRE(h->ready, "bdr_obs_norm_apply before finish / set: there are no statistics yet");
    BDR_REQUIRE(dtype == BDR_DTYPE_F32 || dtype == BDR_DTYPE_F64, "dtype must be BDR_DTYPE_F32 or BDR_DTYPE_F64");
    if (n == 0) return BDR_OK;
    BDR_REQUIRE(rows && out, "null rows");
    const float* mean = h->mean.data(); const float* std = h->std.data();
    for (uint64_t k = 0; k < n; ++k)
        for (uint64_t c = 0; c < h->dim; ++c) {
            const float x = dtype == BDR_DTYPE_F64 ? (float)((const double*)rows)[k * h->dim + c] : ((const float*)rows)[k * h->dim + c];
            out[k * h->dim + c] = obs_norm_z(x, mean[c], std[c]);
        }
    return BDR_OK;
}

int32_t bdr_obs_norm_apply_device(const bdr_obs_norm* h, uint64_t n, const void* rows_dev, uint64_t row_stride, int32_t dtype, float* out_dev,
                                  uint64_t out_stride)
{
    BDR_REQUIRE(h, "null normaliser handle");
    BDR_REQUIRE(h->ready, "bdr_obs_norm_apply_device before finish / set: there are no statistics yet");
    BDR_REQUIRE(dtype == BDR_DTYPE_F32 || dtype == BDR_DTYPE_F64, "dtype must be BDR_DTYPE_F32 or BDR_DTYPE_F64");
    if (n == 0) return BDR_OK;
    BDR_REQUIRE(rows_dev && out_dev, "null rows");
    const uint64_t eb = elem_bytes(dtype);
    BDR_REQUIRE(row_stride >= h->dim * eb && row_stride % eb == 0 && (uintptr_t)rows_dev % eb == 0,
                "row_stride must be a multiple of the element size and >= dim elements, rows_dev aligned to the element size");
    BDR_REQUIRE(out_stride >= h->dim * 4 && out_stride % 4 == 0 && (uintptr_t)out_dev % 4 == 0,
                "out_stride must be a multiple of 4 and >= dim * 4, out_dev aligned to 4");
    BDR_REQUIRE(n < (1ull << 38) / h->dim, "too many rows");
    BDR_HIP(hipSetDevice(h->device));
    for (const void* p : {rows_dev, (const void*)out_dev}) {
        hipPointerAttribute_t at{};
        BDR_REQUIRE(hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == h->device,
                    "rows_dev / out_dev must be device memory of the normaliser's GPU (host rows go through bdr_obs_norm_apply)");
    }
    const uint32_t grid = (uint32_t)((n * h->dim + 255) / 256);
    if (dtype == BDR_DTYPE_F64)
        hipLaunchKernelGGL(k_norm_apply<double>, dim3(grid), dim3(256), 0, h->stream, (const uint8_t*)rows_dev, row_stride, n, h->dim, h->d_meanf, h->d_stdf,
                           (uint8_t*)out_dev, out_stride);
    else
        hipLaunchKernelGGL(k_norm_apply<float>, dim3(grid), dim3(256), 0, h->stream, (const uint8_t*)rows_dev, row_stride, n, h->dim, h->d_meanf, h->d_stdf,
                           (uint8_t*)out_dev, out_stride);
    BDR_HIP(hipGetLastError());
    BDR_HIP(hipStreamSynchronize(h->stream));   // the normaliser's stream is nobody else's: the rows are ready for whatever queue reads them next
    return BDR_OK;
}

}  // extern "C"
