//! Observation statistics and normalisation of an offline dataset on the device: `PenConverter`
//! (`border-minari/src/d4rl/pen/candle.rs:42-161`) behind `bdr_obs_norm_*`.
//!
//! `PenConverter::new` computes the per-column mean and standard deviation over `observations[..T]` of every episode and
//! normalises every observation with them - the rows of the replay buffer (`convert_observation_batch[_next]`, `:104-124`) and
//! the observation the policy acts on (`convert_observation`, `:83-87`).  [`AmdObsNorm`] holds those statistics on the GPU:
//! [`AmdReplayBuffer::push_episode`](crate::AmdReplayBuffer::push_episode) takes it for the ring, [`AmdObsNorm::apply`] /
//! [`AmdObsNorm::apply_device`] for acting.  All three produce the same bits: `(x as f32 - mean) / std`, two separately rounded
//! `f32` operations (ndarray's element-wise `(&obs.0 - &self.mean) / &self.std`, `:71-74`).
//!
//! The statistics are accumulated in `f64` over the `f32`-rounded elements, in a fixed order, and rounded to `f32` once; the
//! reference accumulates in `f32` in ndarray's own order, so mean / std agree with it to rounding, not bit for bit.
use crate::{error::check, ffi};
use anyhow::Result;
use std::os::raw::c_void;

/// Element types an observation row may arrive in: `f64` (what Minari stores, `pyobj_to_arrayd::<f64, f32>`) or `f32`.
pub trait ObsElem: Copy {
    const DTYPE: i32;
}
impl ObsElem for f32 {
    const DTYPE: i32 = ffi::BDR_DTYPE_F32;
}
impl ObsElem for f64 {
    const DTYPE: i32 = ffi::BDR_DTYPE_F64;
}

pub struct AmdObsNorm {
    h: *mut ffi::bdr_obs_norm,
    dim: usize,
}

// SAFETY: the handle owns its HIP stream and buffers; the library sets the device on every entry.  Movable between threads.
unsafe impl Send for AmdObsNorm {}

impl AmdObsNorm {
    /// An empty normaliser for rows of `dim` columns on HIP device `device`.
    pub fn new(device: i32, dim: usize) -> Result<Self> {
        let mut h = std::ptr::null_mut();
        check(unsafe { ffi::bdr_obs_norm_create(device, dim as u64, &mut h) })?;
        Ok(Self { h, dim })
    }

    /// `PenConverter::new` over episodes already in memory: `episodes[k]` is the `[T_k + 1][dim]` observation array of episode
    /// `k`; its last row does not count (`pen/candle.rs:56, 146-152`).
    pub fn from_episodes<X: ObsElem>(device: i32, dim: usize, episodes: &[&[X]]) -> Result<Self> {
        let mut this = Self::new(device, dim)?;
        for obs in episodes {
            anyhow::ensure!(obs.len() % dim == 0 && obs.len() >= dim, "an episode's observations are [T + 1][{}]", dim);
            this.accumulate(&obs[..obs.len() - dim])?;
        }
        this.finish()?;
        Ok(this)
    }

    pub fn handle(&self) -> *mut ffi::bdr_obs_norm {
        self.h
    }

    pub fn dim(&self) -> usize {
        self.dim
    }

    /// Adds `rows` (`[n][dim]`) to the statistics.  An error after [`finish`](Self::finish) or [`set`](Self::set).
    pub fn accumulate<X: ObsElem>(&mut self, rows: &[X]) -> Result<()> {
        anyhow::ensure!(rows.len() % self.dim == 0, "rows are [n][{}]", self.dim);
        check(unsafe { ffi::bdr_obs_norm_accumulate(self.h, (rows.len() / self.dim) as u64, rows.as_ptr() as *const c_void, X::DTYPE) })
    }

    /// `mean_axis(Axis(0))` and `std_axis(Axis(0), 1.0)` (`pen/candle.rs:61-62`).  Fails when fewer than two rows were
    /// accumulated or a column is constant (the reference would fill the buffer with NaN).
    pub fn finish(&mut self) -> Result<()> {
        check(unsafe { ffi::bdr_obs_norm_finish(self.h) })
    }

    /// Statistics computed elsewhere (a saved converter).
    pub fn set(&mut self, mean: &[f32], std: &[f32]) -> Result<()> {
        anyhow::ensure!(mean.len() == self.dim && std.len() == self.dim, "mean / std have {} columns", self.dim);
        check(unsafe { ffi::bdr_obs_norm_set(self.h, mean.as_ptr(), std.as_ptr()) })
    }

    /// `(mean, std, rows accumulated)`.
    pub fn stats(&self) -> Result<(Vec<f32>, Vec<f32>, u64)> {
        let (mut mean, mut std, mut n) = (vec![0f32; self.dim], vec![0f32; self.dim], 0u64);
        check(unsafe { ffi::bdr_obs_norm_get(self.h, mean.as_mut_ptr(), std.as_mut_ptr(), &mut n) })?;
        Ok((mean, std, n))
    }

    /// `convert_observation` (`pen/candle.rs:83-87`) on host rows `[n][dim]`.
    pub fn apply<X: ObsElem>(&self, rows: &[X]) -> Result<Vec<f32>> {
        anyhow::ensure!(rows.len() % self.dim == 0, "rows are [n][{}]", self.dim);
        let mut out = vec![0f32; rows.len()];
        check(unsafe { ffi::bdr_obs_norm_apply(self.h, (rows.len() / self.dim) as u64, rows.as_ptr() as *const c_void, X::DTYPE, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// The same for rows that live in HBM: row `k` of `X` at `rows_dev + k * row_stride` bytes, written as `f32` to
    /// `out_dev + k * out_stride` - the input of the agents' `sample_device`.
    ///
    /// # Safety
    /// Both addresses must be device memory of this normaliser's GPU covering `n` rows at those strides.
    pub unsafe fn apply_device<X: ObsElem>(&self, n: usize, rows_dev: *const c_void, row_stride: usize, out_dev: *mut f32, out_stride: usize) -> Result<()> {
        check(ffi::bdr_obs_norm_apply_device(self.h, n as u64, rows_dev, row_stride as u64, X::DTYPE, out_dev, out_stride as u64))
    }
}

impl Drop for AmdObsNorm {
    fn drop(&mut self) {
        unsafe {
            ffi::bdr_obs_norm_destroy(self.h);
        }
    }
}
