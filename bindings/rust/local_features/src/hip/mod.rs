//! `LocalFeaturesHip`: the role of `LocalFeaturesVulkan` (vulkan/mod.rs:98-131) on the MI355X path.  Same public
//! methods -- `detect_extract_all`, `detect_top_n`, `detect(img, Option<&mut dyn FilterBlobs>)` (vulkan/mod.rs:346-367),
//! same `FeaturesResult` -- over liblf_mkd.so (include/lf_mkd.h).  No Vulkan object is held or needed.
//!
//! New file in the reference tree: `local_features/src/hip/mod.rs` (with `ffi.rs` beside it, `build.rs` in the crate root
//! and the few lines of `lib.rs.diff`).  The build image of this repository has no Rust toolchain, so this file has not
//! been compiled there; `tests/test_rust_binding.py` checks its FFI surface against the header mechanically.
//!
//! What a caller can observe differently from the Vulkan backend:
//!   * keypoints come in a defined order (by blob, then orientation-histogram bin; the reference appends atomically),
//!     blobs too (raster order of the 4x4x4 scan cubes);
//!   * the sampler's bilinear weights are exact f32 (the Vulkan sampler's precision is implementation-defined), the
//!     pyramid mirrors at the content edge;
//!   * the pooling contraction runs on the matrix cores from f16 hi+lo splits (descriptors within 1e-5 relative L2 of the
//!     f32 formulation; `LF_MKD_POOL_F32` selects exact f32 arithmetic at half the speed).
mod device;
pub mod ffi;

use std::ffi::{CStr, CString};

use ndarray::{s, Array2, ArrayView2};

use device::DeviceBuffer;

use crate::vulkan::{BlobLocationsView, FilterBlobs, FilterBlobsOutput};
use crate::{BuildTimeParams, FeatureDetectParams, FeaturesResult, Keypoint, DESCRIPTOR_LEN, MKDPCA};

/// Blobs per block of the reference's extremum buffer (vulkan/mod.rs:279); a custom `FilterBlobs` sees chunks of this size.
const EXTREMUM_BLOCK_LEN: usize = 256;

#[derive(Debug, thiserror::Error)]
#[non_exhaustive]
pub enum Error {
    #[error("illegal argument: {0}")]
    BadArgument(String),
    #[error("HIP runtime: {0}")]
    Hip(String),
    #[error("cannot read PCA model: {0}")]
    Io(String),
    #[error("no usable gfx950 device: {0}")]
    NoDevice(String),
    #[error("RCCL: {0}")]
    Comm(String),
    #[error("liblf_mkd: status {0}: {1}")]
    Other(i32, String),
}

fn last_error(h: *const ffi::lf_mkd) -> String {
    // SAFETY: lf_mkd_last_error returns a NUL-terminated string owned by the handle (or by the thread, for h = null)
    unsafe { CStr::from_ptr(ffi::lf_mkd_last_error(h)) }.to_string_lossy().into_owned()
}

fn check(h: *const ffi::lf_mkd, rc: i32) -> Result<(), Error> {
    match rc {
        ffi::LF_MKD_OK => Ok(()),
        ffi::LF_MKD_ERR_BAD_ARG | ffi::LF_MKD_ERR_NO_IMAGE => Err(Error::BadArgument(last_error(h))),
        ffi::LF_MKD_ERR_HIP => Err(Error::Hip(last_error(h))),
        ffi::LF_MKD_ERR_IO => Err(Error::Io(last_error(h))),
        ffi::LF_MKD_ERR_NO_DEVICE => Err(Error::NoDevice(last_error(h))),
        ffi::LF_MKD_ERR_COMM => Err(Error::Comm(last_error(h))),
        other => Err(Error::Other(other, last_error(h))),
    }
}

// `Keypoint` (lib.rs:17-24) and `lf_mkd_keypoint` are both five f32 in the same order.  `Keypoint` is not `#[repr(C)]`
// in the reference; lib.rs.diff adds the attribute, and these assertions keep the two in step.
const _: () = assert!(std::mem::size_of::<Keypoint>() == std::mem::size_of::<ffi::lf_mkd_keypoint>());
const _: () = assert!(std::mem::align_of::<Keypoint>() == std::mem::align_of::<ffi::lf_mkd_keypoint>());

/// `flags` of `lf_mkd_verify_homography*` and `lf_mkd_verify_fundamental*` (`include/lf_mkd.h`): the best RANSAC
/// candidate as is, no least-squares refit.
pub const VERIFY_NO_REFINE: u32 = 1;

/// `flags` of `lf_mkd_match_pairs_device` (`include/lf_mkd.h`, `LF_MKD_MATCH_MUTUAL`): both directions are matched and a
/// match is kept only if the other direction agrees.
pub const MATCH_MUTUAL: u32 = 1;

/// `kind` of `lf_mkd_match_guided_pairs_device` (`include/lf_mkd.h`, `LF_MKD_GUIDE_HOMOGRAPHY` / `LF_MKD_GUIDE_FUNDAMENTAL`):
/// what a pair's nine model floats are -- the H or the F its verifier wrote.
pub const GUIDE_HOMOGRAPHY: u32 = 0;
pub const GUIDE_FUNDAMENTAL: u32 = 1;

/// `flags` of `lf_mkd_track_table_device` (`include/lf_mkd.h`, `LF_MKD_TRACK_TABLE_CONSISTENT`): only tracks without
/// conflicting rows (`dup == 0`) enter the table.
pub const TRACK_TABLE_CONSISTENT: u32 = 1;

/// `flags` of `lf_mkd_link_table_device` (`include/lf_mkd.h`, `LF_MKD_LINK_TABLE_LOCAL`): the table holds rows local to
/// their images, not pool rows.
pub const LINK_TABLE_LOCAL: u32 = 1;

/// `flags` of `lf_mkd_select_edges_device` (`include/lf_mkd.h`, `LF_MKD_SELECT_SKIP_SELF`, `LF_MKD_SELECT_UNIQUE`): column i
/// is no candidate of row i; one pool, every unordered pair at most once, as (smaller, larger).  `SELECT_MAX_K`: the
/// largest k (`LF_MKD_SELECT_MAX_K`).
pub const SELECT_SKIP_SELF: u32 = 1;
pub const SELECT_UNIQUE: u32 = 2;
pub const SELECT_MAX_K: u32 = 32;

/// `flags` of `lf_mkd_covisibility_device` (`include/lf_mkd.h`, `LF_MKD_COVIS_ACCUMULATE`): the table is added to what
/// `d_covis` holds.
pub const COVIS_ACCUMULATE: u32 = 1;
/// `flags` of `lf_mkd_resect_cameras_device` (`include/lf_mkd.h`, `LF_MKD_RESECT_ALL`): registered images are resected too.
pub const RESECT_ALL: u32 = 1;
/// `refine` of `lf_mkd_bundle_adjust_intrinsics` (`include/lf_mkd.h`, `LF_MKD_BA_REFINE_FOCAL`, `LF_MKD_BA_REFINE_PRINCIPAL`).
pub const BA_REFINE_FOCAL: u32 = 1;
pub const BA_REFINE_PRINCIPAL: u32 = 2;
/// `flags` of `lf_mkd_view_graph` (`include/lf_mkd.h`, `LF_MKD_VIEW_GRAPH_USE_UNCHECKED`): edges that close no triangle are kept.
pub const VIEW_GRAPH_USE_UNCHECKED: u32 = 1;
/// `root` of `lf_mkd_view_graph` (`LF_MKD_VIEW_GRAPH_AUTO_ROOT`): the image with the most kept incident edges.
pub const VIEW_GRAPH_AUTO_ROOT: u32 = 0xFFFF_FFFF;

pub struct LocalFeaturesHip {
    h: *mut ffi::lf_mkd,
    fixed_params: BuildTimeParams,
}

// One handle per thread at a time (`&mut self` on every call, as LocalFeaturesVulkan); it may move between threads.
unsafe impl Send for LocalFeaturesHip {}

impl LocalFeaturesHip {
    /// `LocalFeaturesVulkan::new` + `upload_constant_data` (vulkan/mod.rs:253-323,1587-1713).  The PCA tensors are the
    /// ones `PCAModel::from_safetensors` yields from the embedded model bytes (mkd_ref.rs:26-31,352-391).
    pub fn new(fixed_params: BuildTimeParams, params: FeatureDetectParams, device: i32) -> Result<Self, Error> {
        let bytes = match fixed_params.pca {
            MKDPCA::LIBERTY => crate::mkd_ref::PCA_SAFETENSORS_LIBERTY,
            MKDPCA::NOTREDAME => crate::mkd_ref::PCA_SAFETENSORS_NOTREDAME,
            MKDPCA::YOSEMITE => crate::mkd_ref::PCA_SAFETENSORS_YOSEMITE,
        };
        let pca = crate::mkd_ref::PCAModel::from_safetensors(bytes).map_err(|e| Error::Io(e.to_string()))?;
        let mean = pca.mean.as_standard_layout();
        let eigvals = pca.eigvals.as_standard_layout();
        let eigvecs = pca.eigvecs.as_standard_layout(); // [238][238] row-major, as lf_mkd_create expects
        let p = ffi::lf_mkd_params {
            max_image_width: fixed_params.max_image_width,
            max_image_height: fixed_params.max_image_height,
            max_features: fixed_params.max_features,
            patch_scale_factor: params.patch_scale_factor,
            device,
            angle_mode: ffi::LF_MKD_ANGLE_SHADER,
            pool_mode: ffi::LF_MKD_POOL_DEFAULT,
            n_scales: fixed_params.n_scales,
            max_blobs: fixed_params.max_blobs,
            ..Default::default()
        };
        let mut h: *mut ffi::lf_mkd = std::ptr::null_mut();
        // SAFETY: the three arrays hold 238, 238 and 238*238 contiguous f32 and outlive the call; `h` receives the handle
        let rc = unsafe {
            ffi::lf_mkd_create(&p, mean.as_ptr(), eigvals.as_ptr(), eigvecs.as_ptr(), &mut h)
        };
        check(std::ptr::null(), rc)?;
        Ok(Self { h, fixed_params })
    }

    /// Same, reading `concat-pca-*.safetensors` from a directory (for a build that does not embed the models).
    pub fn from_model_dir(fixed_params: BuildTimeParams, params: FeatureDetectParams, device: i32, dir: &str)
        -> Result<Self, Error> {
        let name = match fixed_params.pca {
            MKDPCA::LIBERTY => "liberty",
            MKDPCA::NOTREDAME => "notredame",
            MKDPCA::YOSEMITE => "yosemite",
        };
        let path = CString::new(format!("{dir}/concat-pca-{name}.safetensors")).map_err(|e| Error::Io(e.to_string()))?;
        let p = ffi::lf_mkd_params {
            max_image_width: fixed_params.max_image_width,
            max_image_height: fixed_params.max_image_height,
            max_features: fixed_params.max_features,
            patch_scale_factor: params.patch_scale_factor,
            device,
            n_scales: fixed_params.n_scales,
            max_blobs: fixed_params.max_blobs,
            ..Default::default()
        };
        let mut h: *mut ffi::lf_mkd = std::ptr::null_mut();
        // SAFETY: `path` is NUL-terminated and outlives the call
        let rc = unsafe { ffi::lf_mkd_create_from_file(&p, path.as_ptr(), &mut h) };
        check(std::ptr::null(), rc)?;
        Ok(Self { h, fixed_params })
    }

    /// vulkan/mod.rs:346-351: every blob the detector finds (at most `max_blobs`).
    pub fn detect_extract_all(&mut self, img: &ArrayView2<f32>) -> Result<FeaturesResult, Error> {
        self.detect_on_device(img, 0, 0.0)
    }

    /// vulkan/mod.rs:353-361: the `n` blobs of largest contrast among those of size >= `min_size`
    /// (`TopKContrastFilter`, vulkan/mod.rs:1753-1786, run on the device).
    pub fn detect_top_n(&mut self, img: &ArrayView2<f32>, n: u32, min_size: f32) -> Result<FeaturesResult, Error> {
        self.detect_on_device(img, n, min_size)
    }

    /// `detect_top_n` on the 8-bit luma the reference's callers convert from (`image::open(..).grayscale()` then `convert()`,
    /// examples/match_images/src/main.rs:44-60; `u8 as f32 / 255.`, examples/webcam/src/main.rs:136): a quarter of the
    /// upload, the same keypoints and descriptors bit for bit (the device divides by 255 with a correctly rounded division).
    pub fn detect_top_n_u8(&mut self, img: &ArrayView2<u8>, n: u32, min_size: f32) -> Result<FeaturesResult, Error> {
        let width: u32 = img.ncols().try_into().map_err(|_| Error::BadArgument("image too wide".into()))?;
        let height: u32 = img.nrows().try_into().map_err(|_| Error::BadArgument("image too tall".into()))?;
        let data = img.as_slice().expect("image must be contiguous row-major"); // vulkan/mod.rs:368
        let cap = self.fixed_params.max_features as usize;
        let mut keypoints = vec![ffi::lf_mkd_keypoint::default(); cap];
        let mut descriptors = Array2::<f32>::zeros((cap, DESCRIPTOR_LEN));
        let (mut m, mut dropped_blobs, mut dropped_features) = (0u64, 0u64, 0u64);
        // SAFETY: `data` holds width*height bytes; the two outputs have room for `cap` rows
        unsafe {
            check(self.h, ffi::lf_mkd_detect_u8(self.h, data.as_ptr(), width, height, n, min_size, keypoints.as_mut_ptr(),
                                                descriptors.as_mut_ptr(), cap as u64, &mut m, &mut dropped_blobs,
                                                &mut dropped_features))?;
        }
        keypoints.truncate(m as usize);
        Ok(FeaturesResult {
            keypoints: keypoints.into_iter().map(to_keypoint).collect(),
            descriptors: descriptors.slice_move(s![..m as usize, ..]),
            dropped_blobs: dropped_blobs as u32,
            dropped_features: dropped_features as u32,
        })
    }

    /// vulkan/mod.rs:363-593 with a caller-supplied blob filter: detect graph, the filter on the host (where the
    /// reference calls it, vulkan/mod.rs:596-691), extract graph on the blobs it kept.  `None` keeps every blob.
    pub fn detect(&mut self, img: &ArrayView2<f32>, filter_keypoints: Option<&mut dyn FilterBlobs>)
        -> Result<FeaturesResult, Error> {
        let Some(filter) = filter_keypoints else {
            return self.detect_extract_all(img);
        };
        let (width, height) = Self::image_dims(img)?;
        let data = img.as_slice().expect("image must be contiguous row-major"); // vulkan/mod.rs:368
        let max_extrema = 256 * ((self.fixed_params.max_blobs as usize + 255) / 256); // vulkan/mod.rs:279-286
        let mut blobs = vec![ffi::lf_mkd_extremum::default(); max_extrema];
        let (mut n_blobs, mut dropped_blobs) = (0u64, 0u64);
        // SAFETY: `data` holds width*height f32; `blobs` has room for max_extrema records
        unsafe {
            check(self.h, ffi::lf_mkd_set_image(self.h, data.as_ptr(), width, height))?;
            check(self.h, ffi::lf_mkd_detect_extrema(self.h, blobs.as_mut_ptr(), max_extrema as u64, &mut n_blobs,
                                                     &mut dropped_blobs))?;
        }
        blobs.truncate(n_blobs as usize);

        // the filter sees the blobs as the reference hands them over: structure of arrays, in blocks of 256
        let xs: Vec<f32> = blobs.iter().map(|b| b.x).collect();
        let ys: Vec<f32> = blobs.iter().map(|b| b.y).collect();
        let scales: Vec<f32> = blobs.iter().map(|b| b.size).collect();
        let contrasts: Vec<f32> = blobs.iter().map(|b| b.response).collect();
        let mut indices: Vec<u32> = Vec::new();
        {
            let views = (0..blobs.len()).step_by(EXTREMUM_BLOCK_LEN).map(|lo| {
                let hi = (lo + EXTREMUM_BLOCK_LEN).min(blobs.len());
                BlobLocationsView { xs: &xs[lo..hi], ys: &ys[lo..hi], scales: &scales[lo..hi], contrasts: &contrasts[lo..hi] }
            });
            filter.filter(Box::new(views), FilterBlobsOutput { indices: &mut indices });
        }
        let mut kept = Vec::with_capacity(indices.len());
        for i in indices {
            let blob = blobs.get(i as usize)
                .ok_or_else(|| Error::BadArgument(format!("FilterBlobs returned index {i} of {} blobs", blobs.len())))?;
            kept.push(*blob);
        }

        let cap = self.fixed_params.max_features as usize;
        let mut keypoints = vec![ffi::lf_mkd_keypoint::default(); cap];
        let (mut n_kp, mut dropped_features) = (0u64, 0u64);
        // SAFETY: `kept` holds kept.len() records, `keypoints` has room for `cap`
        unsafe {
            check(self.h, ffi::lf_mkd_orient_keypoints(self.h, kept.as_ptr(), kept.len() as u64, keypoints.as_mut_ptr(),
                                                       cap as u64, &mut n_kp, &mut dropped_features))?;
        }
        keypoints.truncate(n_kp as usize);
        let mut descriptors = Array2::<f32>::zeros((keypoints.len(), DESCRIPTOR_LEN));
        // SAFETY: `descriptors` is a fresh standard-layout [n_kp][128] array
        unsafe {
            check(self.h, ffi::lf_mkd_describe_keypoints(self.h, keypoints.as_ptr(), n_kp, descriptors.as_mut_ptr()))?;
        }
        Ok(FeaturesResult {
            keypoints: keypoints.into_iter().map(to_keypoint).collect(),
            descriptors,
            dropped_blobs: dropped_blobs as u32,
            dropped_features: dropped_features as u32,
        })
    }

    /// The describe half on its own (the extract graph after orientation, vulkan/mod.rs:1277-1572): descriptors of the
    /// given keypoints on `img`.  The reference has no public call for this; the path's benchmarks use it.
    pub fn describe(&mut self, img: &ArrayView2<f32>, keypoints: &[Keypoint]) -> Result<Array2<f32>, Error> {
        let (width, height) = Self::image_dims(img)?;
        let data = img.as_slice().expect("image must be contiguous row-major");
        let kps: Vec<ffi::lf_mkd_keypoint> = keypoints.iter().map(from_keypoint).collect();
        let mut out = Array2::<f32>::zeros((kps.len(), DESCRIPTOR_LEN));
        // SAFETY: sizes as declared; `out` is standard layout
        unsafe {
            check(self.h, ffi::lf_mkd_set_image(self.h, data.as_ptr(), width, height))?;
            check(self.h, ffi::lf_mkd_describe_keypoints(self.h, kps.as_ptr(), kps.len() as u64, out.as_mut_ptr()))?;
        }
        Ok(out)
    }

    /// `match_features` of examples/match_images/src/main.rs:8-27 (dot-product similarity, Lowe's ratio 0.8).
    pub fn match_features(&mut self, a: &ArrayView2<f32>, b: &ArrayView2<f32>) -> Result<Vec<(usize, usize)>, Error> {
        assert_eq!(a.ncols(), DESCRIPTOR_LEN);
        assert_eq!(b.ncols(), DESCRIPTOR_LEN);
        let (a, b) = (a.as_standard_layout(), b.as_standard_layout());
        let mut m = vec![-1i32; a.nrows()];
        // SAFETY: a, b are contiguous [n][128]; `m` has a.nrows() entries
        unsafe {
            check(self.h, ffi::lf_mkd_match(self.h, a.as_ptr(), a.nrows() as u64, b.as_ptr(), b.nrows() as u64, 0.8,
                                            m.as_mut_ptr()))?;
        }
        Ok(m.iter().enumerate().filter(|(_, j)| **j >= 0).map(|(i, j)| (i, *j as usize)).collect())
    }

    /// 8-bit descriptors (`lf_mkd_quantize_descriptors`, `include/lf_mkd.h`): byte = clamp(rint(x * 256), -127, 127) + 128,
    /// a quarter of the bytes of the f32 rows.
    pub fn quantize(&mut self, desc: &ArrayView2<f32>) -> Result<Array2<u8>, Error> {
        assert_eq!(desc.ncols(), DESCRIPTOR_LEN);
        let desc = desc.as_standard_layout();
        let mut q = Array2::<u8>::zeros((desc.nrows(), DESCRIPTOR_LEN));
        // SAFETY: desc is contiguous [n][128]; `q` is standard layout with as many rows
        unsafe {
            check(self.h, ffi::lf_mkd_quantize_descriptors(self.h, desc.as_ptr(), desc.nrows() as u64, 0.0, q.as_mut_ptr()))?;
        }
        Ok(q)
    }

    /// `match_features` over 8-bit descriptors (`lf_mkd_match_q8`): exact integer similarities, Lowe's ratio 0.8.
    pub fn match_q8(&mut self, a: &ArrayView2<u8>, b: &ArrayView2<u8>) -> Result<Vec<(usize, usize)>, Error> {
        assert_eq!(a.ncols(), DESCRIPTOR_LEN);
        assert_eq!(b.ncols(), DESCRIPTOR_LEN);
        let (a, b) = (a.as_standard_layout(), b.as_standard_layout());
        let mut m = vec![-1i32; a.nrows()];
        // SAFETY: a, b are contiguous [n][128]; `m` has a.nrows() entries
        unsafe {
            check(self.h, ffi::lf_mkd_match_q8(self.h, a.as_ptr(), a.nrows() as u64, b.as_ptr(), b.nrows() as u64, 0.8,
                                               m.as_mut_ptr()))?;
        }
        Ok(m.iter().enumerate().filter(|(_, j)| **j >= 0).map(|(i, j)| (i, *j as usize)).collect())
    }

    /// k-nearest-neighbour search over 8-bit descriptors (`lf_mkd_knn_q8`): for each row of `a` its `k` best rows of `b` as
    /// `(index [na, k], score [na, k])`, larger similarity first and among equal similarities the higher index first; slots
    /// beyond the number of candidates hold `-1` / `i32::MIN`.  `1 <= k <= 16`.
    pub fn knn_q8(&mut self, a: &ArrayView2<u8>, b: &ArrayView2<u8>, k: usize) -> Result<(Array2<i32>, Array2<i32>), Error> {
        assert_eq!(a.ncols(), DESCRIPTOR_LEN);
        assert_eq!(b.ncols(), DESCRIPTOR_LEN);
        let (a, b) = (a.as_standard_layout(), b.as_standard_layout());
        let mut index = Array2::<i32>::from_elem((a.nrows(), k), -1);
        let mut score = Array2::<i32>::from_elem((a.nrows(), k), i32::MIN);
        // SAFETY: a, b are contiguous [n][128]; `index` and `score` have a.nrows() * k entries each
        unsafe {
            check(self.h, ffi::lf_mkd_knn_q8(self.h, a.as_ptr(), a.nrows() as u64, b.as_ptr(), b.nrows() as u64, k as u32,
                                             index.as_mut_ptr(), score.as_mut_ptr()))?;
        }
        Ok((index, score))
    }

    /// The ratio test against the best neighbour from another group over 8-bit descriptors (`lf_mkd_match_q8_grouped`):
    /// `groups_b[j]` is the group (image, object) of row j of `b`.  Returns `(matches, best, rival)`: `matches[i]` is the
    /// best row of `b` for row i of `a`, or -1 when `best * ratio > rival` fails; `rival[i]` is the best score among the rows
    /// whose group differs from the best's, `i32::MIN` if there is none.
    pub fn match_q8_grouped(&mut self, a: &ArrayView2<u8>, b: &ArrayView2<u8>, groups_b: &[u32], ratio: f32)
                            -> Result<(Vec<i32>, Vec<i32>, Vec<i32>), Error> {
        assert_eq!(a.ncols(), DESCRIPTOR_LEN);
        assert_eq!(b.ncols(), DESCRIPTOR_LEN);
        assert_eq!(groups_b.len(), b.nrows());
        let (a, b) = (a.as_standard_layout(), b.as_standard_layout());
        let (mut m, mut best, mut rival) = (vec![-1i32; a.nrows()], vec![i32::MIN; a.nrows()], vec![i32::MIN; a.nrows()]);
        // SAFETY: a, b are contiguous [n][128]; groups_b has b.nrows() entries; the outputs have a.nrows() entries each
        unsafe {
            check(self.h, ffi::lf_mkd_match_q8_grouped(self.h, a.as_ptr(), a.nrows() as u64, b.as_ptr(), b.nrows() as u64,
                                                       groups_b.as_ptr(), ratio, m.as_mut_ptr(), best.as_mut_ptr(),
                                                       rival.as_mut_ptr()))?;
        }
        Ok((m, best, rival))
    }

    /// Many pairs of 8-bit descriptors in one call (`lf_mkd_match_q8_pairs_device`): pair p is rows
    /// `offsets_a[p]..offsets_a[p + 1]` of `a` against rows `offsets_b[p]..offsets_b[p + 1]` of `b` (`n_pairs + 1`
    /// non-decreasing offsets each), every pair decided exactly as `match_q8` decides it alone, Lowe's ratio 0.8.  With
    /// `mutual` a match is kept only if the other direction agrees (`MATCH_MUTUAL`).  Returns, per pair, the (row of the
    /// pair's a rows, row of its b rows) matches.  The rows, the offsets and the result cross the bus once; the matcher is
    /// one launch (three with `mutual`) for all pairs.
    pub fn match_q8_batch(&mut self, a: &ArrayView2<u8>, offsets_a: &[u64], b: &ArrayView2<u8>, offsets_b: &[u64], mutual: bool)
        -> Result<Vec<Vec<(usize, usize)>>, Error> {
        assert_eq!(a.ncols(), DESCRIPTOR_LEN);
        assert_eq!(b.ncols(), DESCRIPTOR_LEN);
        if offsets_a.is_empty() || offsets_a.len() != offsets_b.len() {
            return Err(Error::BadArgument("match_q8_batch: offsets_a and offsets_b need n_pairs + 1 entries each".into()));
        }
        let n_pairs = offsets_a.len() - 1;
        let (a, b) = (a.as_standard_layout(), b.as_standard_layout());
        let (na, nb) = (a.nrows(), b.nrows());
        let mut m = vec![-1i32; na];
        if n_pairs > 0 && na > 0 && nb > 0 {
            // SAFETY: a, b are contiguous [n][128]; device buffers sized as declared; `m` has na entries
            unsafe {
                let (d_a, d_b) = (DeviceBuffer::from_slice(a.as_slice().unwrap())?, DeviceBuffer::from_slice(b.as_slice().unwrap())?);
                let (d_oa, d_ob) = (DeviceBuffer::from_slice(offsets_a)?, DeviceBuffer::from_slice(offsets_b)?);
                let d_ab = DeviceBuffer::from_slice(&m)?;                    // rows outside every pair stay -1
                let d_ba = DeviceBuffer::<i32>::new(if mutual { nb } else { 0 })?;
                check(self.h, ffi::lf_mkd_match_q8_pairs_device(
                    self.h, d_a.as_ptr(), d_oa.as_ptr(), na as u64, d_b.as_ptr(), d_ob.as_ptr(), nb as u64, n_pairs as u32, 0.8,
                    if mutual { MATCH_MUTUAL } else { 0 }, d_ab.as_mut_ptr(),
                    if mutual { d_ba.as_mut_ptr() } else { std::ptr::null_mut() }, std::ptr::null_mut(), std::ptr::null_mut(),
                    std::ptr::null_mut()))?;
                check(self.h, ffi::lf_mkd_synchronize(self.h))?;
                d_ab.download(&mut m)?;
            }
        }
        Ok((0..n_pairs).map(|p| {
            let (lo, hi) = ((offsets_a[p] as usize).min(na), (offsets_a[p + 1] as usize).min(na));
            (lo..hi.max(lo)).filter(|&i| m[i] >= 0).map(|i| (i - lo, m[i] as usize)).collect()
        }).collect())
    }

    /// Any pairs of images from one pool in one call (`lf_mkd_match_q8_edges_device`): image m is rows
    /// `image_offsets[m]..image_offsets[m + 1]` of `q`, and edge (i, j) matches image i against image j, decided exactly as
    /// `match_q8` decides the two images alone, Lowe's ratio 0.8.  An image may sit on any number of edges -- a window, all
    /// i < j, a query against its ranked candidates -- and no descriptor row is copied: the pool crosses the bus once.  With
    /// `mutual` a match is kept only if the other direction agrees.  Returns, per edge, the (row of image i, row of image j)
    /// matches.  The edge layouts (`lf_mkd_edge_layout_device`) are made on the device; the host sizes the outputs from its
    /// own copy of the offsets.
    pub fn match_q8_edges(&mut self, q: &ArrayView2<u8>, image_offsets: &[u64], edges: &[(u32, u32)], mutual: bool)
        -> Result<Vec<Vec<(usize, usize)>>, Error> {
        assert_eq!(q.ncols(), DESCRIPTOR_LEN);
        if image_offsets.is_empty() {
            return Err(Error::BadArgument("match_q8_edges: image_offsets needs n_images + 1 entries".into()));
        }
        let q = q.as_standard_layout();
        let (n, n_images, n_edges) = (q.nrows(), image_offsets.len() - 1, edges.len());
        let rows = |m: u32| -> usize {
            let m = m as usize;
            if m >= n_images { return 0; }
            let (lo, hi) = ((image_offsets[m] as usize).min(n), (image_offsets[m + 1] as usize).min(n));
            hi.max(lo) - lo
        };
        let (ea, eb): (Vec<u32>, Vec<u32>) = edges.iter().copied().unzip();
        let (cap_a, cap_b): (usize, usize) = (ea.iter().map(|&m| rows(m)).sum(), eb.iter().map(|&m| rows(m)).sum());
        let mut m = vec![-1i32; cap_a];
        let mut layout = vec![0u64; n_edges + 1];
        if n_edges > 0 && n > 0 {
            // SAFETY: q is contiguous [n][128]; device buffers sized as declared; the capacities bound what is written
            unsafe {
                let d_q = DeviceBuffer::from_slice(q.as_slice().unwrap())?;
                let d_io = DeviceBuffer::from_slice(image_offsets)?;
                let (d_ea, d_eb) = (DeviceBuffer::from_slice(&ea)?, DeviceBuffer::from_slice(&eb)?);
                let (d_la, d_lb) = (DeviceBuffer::<u64>::new(n_edges + 1)?, DeviceBuffer::<u64>::new(n_edges + 1)?);
                let d_ab = DeviceBuffer::from_slice(&m)?;                    // entries of no edge stay -1
                let d_ba = DeviceBuffer::<i32>::new(if mutual { cap_b } else { 0 })?;
                for (d_e, d_l) in [(&d_ea, &d_la), (&d_eb, &d_lb)] {
                    check(self.h, ffi::lf_mkd_edge_layout_device(self.h, d_io.as_ptr(), n_images as u32, n as u64, d_e.as_ptr(),
                                                                 n_edges as u32, d_l.as_mut_ptr(), std::ptr::null_mut()))?;
                }
                check(self.h, ffi::lf_mkd_match_q8_edges_device(
                    self.h, d_q.as_ptr(), d_io.as_ptr(), n_images as u32, n as u64, d_q.as_ptr(), d_io.as_ptr(), n_images as u32,
                    n as u64, d_ea.as_ptr(), d_eb.as_ptr(), d_la.as_ptr(), cap_a as u64,
                    if mutual { d_lb.as_ptr() } else { std::ptr::null() }, if mutual { cap_b as u64 } else { 0 }, n_edges as u32,
                    0.8, if mutual { MATCH_MUTUAL } else { 0 }, d_ab.as_mut_ptr(),
                    if mutual { d_ba.as_mut_ptr() } else { std::ptr::null_mut() }, std::ptr::null_mut(), std::ptr::null_mut(),
                    std::ptr::null_mut()))?;
                check(self.h, ffi::lf_mkd_synchronize(self.h))?;
                d_ab.download(&mut m)?;
                d_la.download(&mut layout)?;
            }
        }
        Ok((0..n_edges).map(|e| {
            let (lo, hi) = ((layout[e] as usize).min(cap_a), (layout[e + 1] as usize).min(cap_a));
            (lo..hi.max(lo)).filter(|&i| m[i] >= 0).map(|i| (i - lo, m[i] as usize)).collect()
        }).collect())
    }

    /// The tracks of a matched collection (`lf_mkd_build_tracks_device`): the connected components of the matches
    /// `match_q8_edges` returned for `edges` over the pool `image_offsets` describes (`n_rows` rows).  Returns, per pool row,
    /// (track, length, dup): the smallest pool row of the row's component, and -- at a row that is a label, 0 elsewhere -- the
    /// rows of the track and its conflicting rows (the rows beyond the first that one image has in it; 0: a consistent
    /// track).  A row on no match is its own track of length 1.
    pub fn build_tracks(&mut self, n_rows: usize, image_offsets: &[u64], edges: &[(u32, u32)], matches: &[Vec<(usize, usize)>])
        -> Result<(Vec<i32>, Vec<u32>, Vec<u32>), Error> {
        if image_offsets.is_empty() || matches.len() != edges.len() {
            return Err(Error::BadArgument("build_tracks: image_offsets needs n_images + 1 entries, matches one list per edge".into()));
        }
        let (n_images, n_edges) = (image_offsets.len() - 1, edges.len());
        let rows = |m: u32| -> usize {
            let m = m as usize;
            if m >= n_images { return 0; }
            let (lo, hi) = ((image_offsets[m] as usize).min(n_rows), (image_offsets[m + 1] as usize).min(n_rows));
            hi.max(lo) - lo
        };
        let (ea, eb): (Vec<u32>, Vec<u32>) = edges.iter().copied().unzip();
        // the a side's edge layout and the match array in it, from the host's own copy of the offsets
        let mut layout = vec![0u64; n_edges + 1];
        for e in 0..n_edges { layout[e + 1] = layout[e] + rows(ea[e]) as u64; }
        let cap = layout[n_edges] as usize;
        let mut m = vec![-1i32; cap];
        for (e, list) in matches.iter().enumerate() {
            for &(i, j) in list {
                if i < rows(ea[e]) { m[layout[e] as usize + i] = j as i32; }
            }
        }
        let (mut track, mut len, mut dup) = (vec![0i32; n_rows], vec![0u32; n_rows], vec![0u32; n_rows]);
        if n_rows > 0 {
            // SAFETY: device buffers sized as declared; n_rows and cap bound what is read and written
            unsafe {
                let d_io = DeviceBuffer::from_slice(image_offsets)?;
                let (d_ea, d_eb) = (DeviceBuffer::from_slice(&ea)?, DeviceBuffer::from_slice(&eb)?);
                let d_la = DeviceBuffer::from_slice(&layout)?;
                let d_m = DeviceBuffer::from_slice(&m)?;
                let d_track = DeviceBuffer::<i32>::new(n_rows)?;
                let (d_len, d_dup) = (DeviceBuffer::<u32>::new(n_rows)?, DeviceBuffer::<u32>::new(n_rows)?);
                check(self.h, ffi::lf_mkd_build_tracks_device(
                    self.h, d_io.as_ptr(), n_images as u32, n_rows as u64, d_ea.as_ptr(), d_eb.as_ptr(), d_la.as_ptr(),
                    cap as u64, n_edges as u32, d_m.as_ptr(), 0, d_track.as_mut_ptr(), d_len.as_mut_ptr(), d_dup.as_mut_ptr(),
                    std::ptr::null_mut()))?;
                check(self.h, ffi::lf_mkd_synchronize(self.h))?;
                d_track.download(&mut track)?;
                d_len.download(&mut len)?;
                d_dup.download(&mut dup)?;
            }
        }
        Ok((track, len, dup))
    }

    /// The track table of `build_tracks`' result (`lf_mkd_track_table_device`): the tracks of at least `min_len` rows -- with
    /// `consistent` only those without conflicting rows -- in the order of their smallest row, as a CSR table.  Returns
    /// (offsets, rows, images): track i's observations are `rows[offsets[i] .. offsets[i + 1]]`, ascending pool rows, and
    /// `images` holds the image of each (`u32::MAX`: a row of no image).
    pub fn track_table(&mut self, image_offsets: &[u64], track: &[i32], len: &[u32], dup: &[u32], min_len: u32, consistent: bool)
        -> Result<(Vec<u64>, Vec<i32>, Vec<u32>), Error> {
        let n = track.len();
        if image_offsets.is_empty() || len.len() != n || dup.len() != n || min_len == 0 {
            return Err(Error::BadArgument("track_table: image_offsets needs n_images + 1 entries, len and dup one entry per row, min_len >= 1".into()));
        }
        if n == 0 { return Ok((vec![0], Vec::new(), Vec::new())); }
        let track_cap = n / min_len as usize;
        let mut counts = [0u32; 4];
        let (mut offsets, mut rows, mut images) = (vec![0u64; track_cap + 1], vec![0i32; n], vec![0u32; n]);
        // SAFETY: device buffers sized as declared; n and the two capacities bound what is read and written
        unsafe {
            let d_io = DeviceBuffer::from_slice(image_offsets)?;
            let (d_track, d_len, d_dup) = (DeviceBuffer::from_slice(track)?, DeviceBuffer::from_slice(len)?, DeviceBuffer::from_slice(dup)?);
            let d_off = DeviceBuffer::<u64>::new(track_cap + 1)?;
            let (d_rows, d_images) = (DeviceBuffer::<i32>::new(n)?, DeviceBuffer::<u32>::new(n)?);
            let d_counts = DeviceBuffer::<u32>::new(4)?;
            check(self.h, ffi::lf_mkd_track_table_device(
                self.h, d_io.as_ptr(), (image_offsets.len() - 1) as u32, n as u64, d_track.as_ptr(), d_len.as_ptr(), d_dup.as_ptr(),
                min_len, if consistent { TRACK_TABLE_CONSISTENT } else { 0 }, track_cap as u64, n as u64, d_off.as_mut_ptr(),
                d_rows.as_mut_ptr(), d_images.as_mut_ptr(), std::ptr::null_mut(), d_counts.as_mut_ptr(), std::ptr::null_mut()))?;
            check(self.h, ffi::lf_mkd_synchronize(self.h))?;
            d_counts.download(&mut counts)?;
            d_off.download(&mut offsets)?;
            d_rows.download(&mut rows)?;
            d_images.download(&mut images)?;
        }
        offsets.truncate(counts[0] as usize + 1);
        rows.truncate(counts[1] as usize);
        images.truncate(counts[1] as usize);
        Ok((offsets, rows, images))
    }

    /// The covisibility table of a track table (`lf_mkd_covisibility_device`): `offsets` and `images` are what `track_table`
    /// returned; entry `[i * n_images + j]` of the result is the number of tracks images i and j both see, `[i * n_images + i]`
    /// the number of tracks image i sees.  The two entries of every pair in `masked` (the pairs a round of matching used) are
    /// set to 0, so that what is left are the pairs that share tracks without having been matched.
    pub fn covisibility(&mut self, offsets: &[u64], images: &[u32], n_images: usize, masked: &[(u32, u32)])
                        -> Result<Vec<u32>, Error> {
        if offsets.is_empty() || n_images * n_images > i32::MAX as usize {
            return Err(Error::BadArgument("covisibility: offsets needs tracks + 1 entries, n_images^2 must be below 2^31".into()));
        }
        let mut covis = vec![0u32; n_images * n_images];
        if n_images == 0 { return Ok(covis); }
        let counts = [(offsets.len() - 1) as u32, images.len() as u32, 0, 0];
        let (ea, eb): (Vec<u32>, Vec<u32>) = masked.iter().cloned().unzip();
        // SAFETY: device buffers sized as declared; the capacities, n_edges and n_images bound what is read and written
        unsafe {
            let d_off = DeviceBuffer::from_slice(offsets)?;
            let d_images = DeviceBuffer::from_slice(if images.is_empty() { &[0u32][..] } else { images })?;
            let d_counts = DeviceBuffer::from_slice(&counts)?;
            let (d_ea, d_eb) = (DeviceBuffer::from_slice(if ea.is_empty() { &[0u32][..] } else { &ea[..] })?,
                                DeviceBuffer::from_slice(if eb.is_empty() { &[0u32][..] } else { &eb[..] })?);
            let d_covis = DeviceBuffer::<u32>::new(covis.len())?;
            check(self.h, ffi::lf_mkd_covisibility_device(
                self.h, d_off.as_ptr(), (offsets.len() - 1) as u64, d_images.as_ptr(), images.len() as u64, d_counts.as_ptr(),
                n_images as u32, d_ea.as_ptr(), d_eb.as_ptr(), ea.len() as u64, 0, d_covis.as_mut_ptr(), std::ptr::null_mut()))?;
            check(self.h, ffi::lf_mkd_synchronize(self.h))?;
            d_covis.download(&mut covis)?;
        }
        Ok(covis)
    }

    /// The relative pose of one calibrated pair from its fundamental matrix (`lf_mkd_two_view_pose`): `f` is row-major with
    /// b^T F a = 0 in pixels, `k_a` / `k_b` are (fx, fy, cx, cy), `matches` the verified (i, j) pairs.  Returns `None` if there
    /// is no pose, else (R row-major, t with |t| = 1, [links in front, the best other candidate's, the candidate, links with at
    /// least `min_parallax_deg` of parallax], E's singular values over the largest, and per keypoint of a its triangulated
    /// point in camera a's frame with the cosine of the parallax angle, (0, 0, 0, 2) where there is none): x_b = R x_a + t.
    #[allow(clippy::type_complexity)]
    pub fn two_view_pose(&mut self, f: &[f32; 9], k_a: &[f32; 4], k_b: &[f32; 4], kps_a: &[ffi::lf_mkd_keypoint],
                         kps_b: &[ffi::lf_mkd_keypoint], matches: &[(usize, usize)], min_parallax_deg: f32)
                         -> Result<Option<([f32; 9], [f32; 3], [u32; 4], [f32; 3], Vec<[f32; 4]>)>, Error> {
        let mut m = vec![-1i32; kps_a.len()];
        for &(i, j) in matches {
            if i >= kps_a.len() || j >= kps_b.len() {
                return Err(Error::BadArgument("two_view_pose: a match outside the keypoint lists".into()));
            }
            m[i] = j as i32;
        }
        let (mut r, mut t, mut stats, mut sigma) = ([0f32; 9], [0f32; 3], [0u32; 4], [0f32; 3]);
        let mut points = vec![[0f32; 4]; kps_a.len().max(1)];
        // SAFETY: host arrays sized as declared; na and nb bound what is read, points has one row per keypoint of a
        unsafe {
            check(self.h, ffi::lf_mkd_two_view_pose(
                self.h, f.as_ptr(), k_a.as_ptr(), k_b.as_ptr(), kps_a.as_ptr(), kps_a.len() as u64, kps_b.as_ptr(),
                kps_b.len() as u64, m.as_ptr(), min_parallax_deg, 0, r.as_mut_ptr(), t.as_mut_ptr(), stats.as_mut_ptr(),
                sigma.as_mut_ptr(), points.as_mut_ptr() as *mut f32))?;
        }
        points.truncate(kps_a.len());
        Ok(if stats[2] == u32::MAX { None } else { Some((r, t, stats, sigma, points)) })
    }

    /// The 3-D point of every track of a track table under known camera poses (`lf_mkd_triangulate_tracks`): `kps` is the
    /// pool, track i's observations are `obs_row` / `obs_image[offsets[i] .. offsets[i + 1]]`, `intrinsics` holds (fx, fy, cx,
    /// cy) and `poses` R row-major then t per image, world to camera (x_cam = R X + t); an image whose R is all zero is not
    /// registered.  Returns per track (the point with the cosine of its parallax angle, (0, 0, 0, 2) for none; [usable
    /// observations, inliers, reason, the winning pair]; [rms, largest] inlier reprojection error in px) and per observation
    /// its state (0 not usable, 1 usable, 2 inlier).
    #[allow(clippy::type_complexity)]
    pub fn triangulate_tracks(&mut self, kps: &[ffi::lf_mkd_keypoint], offsets: &[u64], obs_row: &[i32], obs_image: &[u32],
                              intrinsics: &[[f32; 4]], poses: &[[f32; 12]], max_reproj_px: f32, rounds: u32)
                              -> Result<(Vec<[f32; 4]>, Vec<[u32; 4]>, Vec<[f32; 2]>, Vec<u32>), Error> {
        if offsets.is_empty() || obs_row.len() != obs_image.len() || intrinsics.len() != poses.len() {
            return Err(Error::BadArgument("triangulate_tracks: offsets needs n_tracks + 1 entries, obs_row and obs_image one \
                                           entry per observation, intrinsics and poses one row per image".into()));
        }
        let n = offsets.len() - 1;
        let (mut points, mut stats, mut err) = (vec![[0f32; 4]; n.max(1)], vec![[0u32; 4]; n.max(1)], vec![[0f32; 2]; n.max(1)]);
        let mut state = vec![0u32; obs_row.len().max(1)];
        // SAFETY: host arrays sized as declared; the counts bound what is read, the outputs have one row per track / observation
        unsafe {
            check(self.h, ffi::lf_mkd_triangulate_tracks(
                self.h, kps.as_ptr(), kps.len() as u64, offsets.as_ptr(), n as u64, obs_row.as_ptr(), obs_image.as_ptr(),
                obs_row.len() as u64, intrinsics.as_ptr() as *const f32, poses.as_ptr() as *const f32, intrinsics.len() as u32,
                max_reproj_px, rounds, 0, points.as_mut_ptr() as *mut f32, stats.as_mut_ptr() as *mut u32,
                err.as_mut_ptr() as *mut f32, state.as_mut_ptr()))?;
        }
        points.truncate(n);
        stats.truncate(n);
        err.truncate(n);
        state.truncate(obs_row.len());
        Ok((points, stats, err, state))
    }

    /// The absolute pose of ONE image from the keypoints it owns in tracks that have a 3-D point (`lf_mkd_resect_camera`):
    /// `kps` are the image's rows, `row_track[r]` the index into `points` of row r's track or -1, `points` X, Y, Z and the
    /// parallax cosine per track ((0, 0, 0, 2): none), `intrinsics` (fx, fy, cx, cy).  P3P samples scored by reprojection
    /// inliers at `max_reproj_px`, `rounds` (0 .. 4) Gauss-Newton steps, kept with at least max(`min_inliers`, 3) inliers.
    /// Returns (R row-major then t, world to camera, all zero for none; [correspondences, inliers, reason, the winning
    /// candidate]; [rms, largest] inlier reprojection error in px) and per row its state (0 no correspondence, 1
    /// correspondence, 2 inlier).
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn resect_camera(&mut self, kps: &[ffi::lf_mkd_keypoint], row_track: &[i32], points: &[[f32; 4]], intrinsics: &[f32; 4],
                         max_reproj_px: f32, min_parallax_deg: f32, n_samples: u32, min_inliers: u32, rounds: u32, seed: u32)
                         -> Result<([f32; 12], [u32; 4], [f32; 2], Vec<u32>), Error> {
        if row_track.len() != kps.len() {
            return Err(Error::BadArgument("resect_camera: row_track needs one entry per row of kps".into()));
        }
        let (mut pose, mut stats, mut err) = ([0f32; 12], [0u32; 4], [0f32; 2]);
        let mut state = vec![0u32; kps.len().max(1)];
        // SAFETY: host arrays sized as declared; the counts bound what is read, the outputs have their stated sizes
        unsafe {
            check(self.h, ffi::lf_mkd_resect_camera(
                self.h, kps.as_ptr(), kps.len() as u64, row_track.as_ptr(), points.as_ptr() as *const f32, points.len() as u64,
                intrinsics.as_ptr(), max_reproj_px, min_parallax_deg, n_samples, min_inliers, rounds, seed, 0,
                pose.as_mut_ptr(), stats.as_mut_ptr(), err.as_mut_ptr(), state.as_mut_ptr()))?;
        }
        state.truncate(kps.len());
        Ok((pose, stats, err, state))
    }

    /// Bundle adjustment (`lf_mkd_bundle_adjust`): the registered cameras of `poses` (R row-major then t per image, an all-zero R
    /// for an image that is not registered) that `camera_fixed` does not mark, and the points of the tracks, refined jointly by
    /// `iterations` (1 .. 64) Levenberg-Marquardt steps on the reprojection error, each solving the reduced camera system by at
    /// most `cg_iterations` (1 .. 256) preconditioned conjugate-gradient steps to `cg_tol`.  `kps` is the pool and
    /// `image_offsets` its image ranges; the track table is `track_offsets`, `obs_row`, `obs_image`; `points` X, Y, Z and the
    /// parallax cosine per track; `obs_state`, if given, is `triangulate_tracks`' (only its inliers are used).
    /// Returns (poses, points, the state of every observation: 0 inactive, 1 active, 2 inlier; the trace: per iteration
    /// [cost, the candidate's cost, lambda, accepted, CG steps, inliers, held cameras, held points]; [free cameras, free
    /// points, active observations, accepted steps]).
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn bundle_adjust(&mut self, kps: &[ffi::lf_mkd_keypoint], image_offsets: &[u64], track_offsets: &[u64], obs_row: &[i32],
                         obs_image: &[u32], points: &[[f32; 4]], intrinsics: &[[f32; 4]], poses: &[[f32; 12]],
                         obs_state: Option<&[u32]>, camera_fixed: Option<&[u32]>, max_reproj_px: f32, lambda0: f32,
                         iterations: u32, cg_iterations: u32, cg_tol: f32)
                         -> Result<(Vec<[f32; 12]>, Vec<[f32; 4]>, Vec<u32>, Vec<[f64; 8]>, [u32; 4]), Error> {
        let (n_images, n_tracks, n_obs) = (intrinsics.len(), points.len(), obs_row.len());
        if image_offsets.len() != n_images + 1 || track_offsets.len() != n_tracks + 1 || obs_image.len() != n_obs
            || poses.len() != n_images || obs_state.map_or(false, |s| s.len() != n_obs)
            || camera_fixed.map_or(false, |f| f.len() != n_images) {
            return Err(Error::BadArgument("bundle_adjust: image_offsets needs n_images + 1 entries, track_offsets n_tracks + 1, \
                                           obs_row, obs_image and obs_state one entry per observation, intrinsics, poses and \
                                           camera_fixed one row per image".into()));
        }
        let mut poses_out = vec![[0f32; 12]; n_images.max(1)];
        let mut points_out = vec![[0f32; 4]; n_tracks.max(1)];
        let mut state = vec![0u32; n_obs.max(1)];
        let mut trace = vec![[0f64; 8]; iterations.max(1) as usize];
        let mut counts = [0u32; 4];
        // SAFETY: host arrays sized as declared; the counts bound what is read, the outputs have their stated sizes
        unsafe {
            check(self.h, ffi::lf_mkd_bundle_adjust(
                self.h, kps.as_ptr(), image_offsets.as_ptr(), n_images as u32, kps.len() as u64, track_offsets.as_ptr(),
                n_tracks as u64, obs_row.as_ptr(), obs_image.as_ptr(), n_obs as u64, points.as_ptr() as *const f32,
                intrinsics.as_ptr() as *const f32, poses.as_ptr() as *const f32,
                obs_state.map_or(std::ptr::null(), |s| s.as_ptr()), camera_fixed.map_or(std::ptr::null(), |f| f.as_ptr()),
                max_reproj_px, lambda0, iterations, cg_iterations, cg_tol, 0, poses_out.as_mut_ptr() as *mut f32,
                points_out.as_mut_ptr() as *mut f32, state.as_mut_ptr(), trace.as_mut_ptr() as *mut f64, counts.as_mut_ptr()))?;
        }
        poses_out.truncate(n_images);
        points_out.truncate(n_tracks);
        state.truncate(n_obs);
        Ok((poses_out, points_out, state, trace, counts))
    }

    /// Self-calibrating bundle adjustment (`lf_mkd_bundle_adjust_intrinsics`): `bundle_adjust` with the intrinsics of the images
    /// that share a lens refined beside the poses and the points.  `camera_group` names the lens of every image (`None`: one
    /// lens; an id >= `n_groups`: that image's intrinsics stay); `refine` is `BA_REFINE_FOCAL | BA_REFINE_PRINCIPAL`: a group's
    /// focal lengths are scaled by one factor s, its principal points shifted by one (dx, dy).
    /// Returns (poses, points, intrinsics, the groups' (s, dx, dy), the states, the trace: `bundle_adjust`'s eight and the held
    /// groups; `bundle_adjust`'s four counts and the free groups).
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn bundle_adjust_intrinsics(&mut self, kps: &[ffi::lf_mkd_keypoint], image_offsets: &[u64], track_offsets: &[u64],
                                    obs_row: &[i32], obs_image: &[u32], points: &[[f32; 4]], intrinsics: &[[f32; 4]],
                                    poses: &[[f32; 12]], obs_state: Option<&[u32]>, camera_fixed: Option<&[u32]>,
                                    camera_group: Option<&[u32]>, n_groups: u32, refine: u32, max_reproj_px: f32, lambda0: f32,
                                    iterations: u32, cg_iterations: u32, cg_tol: f32)
                                    -> Result<(Vec<[f32; 12]>, Vec<[f32; 4]>, Vec<[f32; 4]>, Vec<[f32; 3]>, Vec<u32>, Vec<[f64; 9]>,
                                               [u32; 5]), Error> {
        let (n_images, n_tracks, n_obs) = (intrinsics.len(), points.len(), obs_row.len());
        if image_offsets.len() != n_images + 1 || track_offsets.len() != n_tracks + 1 || obs_image.len() != n_obs
            || poses.len() != n_images || obs_state.map_or(false, |s| s.len() != n_obs)
            || camera_fixed.map_or(false, |f| f.len() != n_images) || camera_group.map_or(false, |g| g.len() != n_images) {
            return Err(Error::BadArgument("bundle_adjust_intrinsics: image_offsets needs n_images + 1 entries, track_offsets                                            n_tracks + 1, obs_row, obs_image and obs_state one entry per observation, intrinsics,                                            poses, camera_fixed and camera_group one row per image".into()));
        }
        let mut poses_out = vec![[0f32; 12]; n_images.max(1)];
        let mut points_out = vec![[0f32; 4]; n_tracks.max(1)];
        let mut intrinsics_out = vec![[0f32; 4]; n_images.max(1)];
        let mut groups = vec![[0f32; 3]; (n_groups as usize).max(1)];
        let mut state = vec![0u32; n_obs.max(1)];
        let mut trace = vec![[0f64; 9]; iterations.max(1) as usize];
        let mut counts = [0u32; 5];
        // SAFETY: host arrays sized as declared; the counts bound what is read, the outputs have their stated sizes
        unsafe {
            check(self.h, ffi::lf_mkd_bundle_adjust_intrinsics(
                self.h, kps.as_ptr(), image_offsets.as_ptr(), n_images as u32, kps.len() as u64, track_offsets.as_ptr(),
                n_tracks as u64, obs_row.as_ptr(), obs_image.as_ptr(), n_obs as u64, points.as_ptr() as *const f32,
                intrinsics.as_ptr() as *const f32, poses.as_ptr() as *const f32,
                obs_state.map_or(std::ptr::null(), |s| s.as_ptr()), camera_fixed.map_or(std::ptr::null(), |f| f.as_ptr()),
                camera_group.map_or(std::ptr::null(), |g| g.as_ptr()), n_groups, refine, max_reproj_px, lambda0, iterations,
                cg_iterations, cg_tol, 0, poses_out.as_mut_ptr() as *mut f32, points_out.as_mut_ptr() as *mut f32,
                intrinsics_out.as_mut_ptr() as *mut f32, groups.as_mut_ptr() as *mut f32, state.as_mut_ptr(),
                trace.as_mut_ptr() as *mut f64, counts.as_mut_ptr()))?;
        }
        poses_out.truncate(n_images);
        points_out.truncate(n_tracks);
        intrinsics_out.truncate(n_images);
        groups.truncate(n_groups as usize);
        state.truncate(n_obs);
        Ok((poses_out, points_out, intrinsics_out, groups, state, trace, counts))
    }

    /// View-graph checks (`lf_mkd_view_graph`): the triangle vote over the posed `edges` (`rotations` and `pose_stats` as
    /// `two_view_pose` returned them, one row per edge), global rotations of the `n_images` images by a breadth-first tree of
    /// `tree_rounds` rounds and `iterations` sweeps of quaternion averaging over the kept edges.  `root` is an image id or
    /// `VIEW_GRAPH_AUTO_ROOT`; `use_unchecked` keeps the edges that close no triangle too.
    /// Returns (rotations, edge stats = closed, consistent, state, representative; the residual cosines; image stats = kept
    /// edges, round, tree edge, rejected edges; counts = usable, supported, rejected, unchecked, kept, labelled, root, 0).
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn view_graph(&mut self, edges: &[(u32, u32)], rotations: &[[f32; 9]], pose_stats: &[[u32; 4]], n_images: u32,
                      max_loop_deg: f32, min_front: u32, root: u32, tree_rounds: u32, iterations: u32, use_unchecked: bool)
                      -> Result<(Vec<[f32; 9]>, Vec<[u32; 4]>, Vec<f32>, Vec<[u32; 4]>, [u32; 8]), Error> {
        let n_edges = edges.len();
        if rotations.len() != n_edges || pose_stats.len() != n_edges {
            return Err(Error::BadArgument("view_graph: rotations and pose_stats need one row per edge".into()));
        }
        let edge_a: Vec<u32> = edges.iter().map(|e| e.0).collect();
        let edge_b: Vec<u32> = edges.iter().map(|e| e.1).collect();
        let mut out = vec![[0f32; 9]; (n_images as usize).max(1)];
        let mut edge_stats = vec![[0u32; 4]; n_edges.max(1)];
        let mut residual = vec![2f32; n_edges.max(1)];
        let mut image_stats = vec![[0u32; 4]; (n_images as usize).max(1)];
        let mut counts = [0u32; 8];
        // SAFETY: host arrays sized as declared; n_edges and n_images bound what is read and written
        unsafe {
            check(self.h, ffi::lf_mkd_view_graph(
                self.h, edge_a.as_ptr(), edge_b.as_ptr(), n_edges as u32, rotations.as_ptr() as *const f32,
                pose_stats.as_ptr() as *const u32, n_images, max_loop_deg, min_front, root, tree_rounds, iterations,
                if use_unchecked { VIEW_GRAPH_USE_UNCHECKED } else { 0 }, std::ptr::null(), 0, std::ptr::null(),
                std::ptr::null_mut(), out.as_mut_ptr() as *mut f32, edge_stats.as_mut_ptr() as *mut u32, residual.as_mut_ptr(),
                image_stats.as_mut_ptr() as *mut u32, counts.as_mut_ptr()))?;
        }
        out.truncate(n_images as usize);
        edge_stats.truncate(n_edges);
        residual.truncate(n_edges);
        image_stats.truncate(n_images as usize);
        Ok((out, edge_stats, residual, image_stats, counts))
    }

    /// Initial poses from the view graph's tree (`lf_mkd_tree_poses`): `rotations` and `image_stats` as `view_graph` returned
    /// them, `edges` and `translations` as `two_view_pose` returned them.  Every labelled image gets its rotation and a centre
    /// one unit step from its tree parent's; an image whose chain does not reach the root within `max_depth` steps gets the
    /// all-zero row.  What `global_positions` starts from.
    pub fn tree_poses(&mut self, edges: &[(u32, u32)], translations: &[[f32; 3]], rotations: &[[f32; 9]],
                      image_stats: &[[u32; 4]], max_depth: u32) -> Result<Vec<[f32; 12]>, Error> {
        let (n_edges, n_images) = (edges.len(), rotations.len());
        if translations.len() != n_edges || image_stats.len() != n_images {
            return Err(Error::BadArgument("tree_poses: translations need one row per edge, image_stats one per rotation".into()));
        }
        let edge_a: Vec<u32> = edges.iter().map(|e| e.0).collect();
        let edge_b: Vec<u32> = edges.iter().map(|e| e.1).collect();
        let mut poses = vec![[0f32; 12]; n_images.max(1)];
        // SAFETY: host arrays sized as declared; n_edges and n_images bound what is read and written
        unsafe {
            check(self.h, ffi::lf_mkd_tree_poses(
                self.h, edge_a.as_ptr(), edge_b.as_ptr(), translations.as_ptr() as *const f32, n_edges as u32,
                rotations.as_ptr() as *const f32, image_stats.as_ptr() as *const u32, n_images as u32, max_depth,
                poses.as_mut_ptr() as *mut f32))?;
        }
        poses.truncate(n_images);
        Ok(poses)
    }

    /// Global positioning (`lf_mkd_global_positions`): all camera centres and all track points at once under the rotations of
    /// `poses`, by `sweeps` alternations of the points' and the cameras' weighted 3x3 solves (unit weights for the first
    /// `warm`, then weights floored at the sine of `robust_deg`), each followed by a similarity that puts the centres'
    /// centroid at 0 and their rms radius at 1.
    /// Returns (poses, points = X, Y, Z, smallest cosine; the observations' states; image stats = usable rows, weighted rows,
    /// sweeps held, reason; the trace = cost, weighted observations, held cameras, unsolved points; the eight counts).
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn global_positions(&mut self, kps: &[ffi::lf_mkd_keypoint], image_offsets: &[u64], track_offsets: &[u64],
                            obs_row: &[i32], obs_image: &[u32], row_track: &[i32], intrinsics: &[[f32; 4]], poses: &[[f32; 12]],
                            sweeps: u32, warm: u32, robust_deg: f32, min_obs: u32)
                            -> Result<(Vec<[f32; 12]>, Vec<[f32; 4]>, Vec<u32>, Vec<[u32; 4]>, Vec<[f64; 4]>, [u32; 8]), Error> {
        let (n_images, n_obs) = (intrinsics.len(), obs_row.len());
        if image_offsets.len() != n_images + 1 || track_offsets.is_empty() || obs_image.len() != n_obs || poses.len() != n_images
            || row_track.len() != kps.len() {
            return Err(Error::BadArgument("global_positions: the arrays' lengths do not agree (include/lf_mkd.h)".into()));
        }
        let n_tracks = track_offsets.len() - 1;
        let mut poses_out = vec![[0f32; 12]; n_images.max(1)];
        let mut points_out = vec![[0f32; 4]; n_tracks.max(1)];
        let mut state = vec![0u32; n_obs.max(1)];
        let mut image_stats = vec![[0u32; 4]; n_images.max(1)];
        let mut trace = vec![[0f64; 4]; sweeps.max(1) as usize];
        let mut counts = [0u32; 8];
        // SAFETY: host arrays sized as declared; the counts bound what is read, the outputs have their stated sizes
        unsafe {
            check(self.h, ffi::lf_mkd_global_positions(
                self.h, kps.as_ptr(), image_offsets.as_ptr(), n_images as u32, kps.len() as u64, track_offsets.as_ptr(),
                n_tracks as u64, obs_row.as_ptr(), obs_image.as_ptr(), n_obs as u64, row_track.as_ptr(),
                intrinsics.as_ptr() as *const f32, poses.as_ptr() as *const f32, sweeps, warm, robust_deg, min_obs, 0,
                poses_out.as_mut_ptr() as *mut f32, points_out.as_mut_ptr() as *mut f32, state.as_mut_ptr(),
                image_stats.as_mut_ptr() as *mut u32, trace.as_mut_ptr() as *mut f64, counts.as_mut_ptr()))?;
        }
        poses_out.truncate(n_images);
        points_out.truncate(n_tracks);
        state.truncate(n_obs);
        image_stats.truncate(n_images);
        trace.truncate(sweeps as usize);
        Ok((poses_out, points_out, state, image_stats, trace, counts))
    }

    /// The link table of a matched collection (`lf_mkd_link_table_device`): per edge the compact list of the matches
    /// `match_q8_edges` or a verifier returned for `edges` over the pool `image_offsets` describes (`n_rows` rows), edges with
    /// fewer than `min_links` of them left out.  Returns (offsets, link_a, link_b, edge_links): edge e's correspondences are
    /// `link_a[offsets[e] .. offsets[e + 1]]` and `link_b[..]`, pool rows -- with `local` rows within their images -- in
    /// ascending row of a; an edge that is not kept has an empty range; `edge_links[e]` is every edge's own count.
    pub fn link_table(&mut self, n_rows: usize, image_offsets: &[u64], edges: &[(u32, u32)], matches: &[Vec<(usize, usize)>],
                      min_links: u32, local: bool) -> Result<(Vec<u64>, Vec<i32>, Vec<i32>, Vec<u32>), Error> {
        if image_offsets.is_empty() || matches.len() != edges.len() {
            return Err(Error::BadArgument("link_table: image_offsets needs n_images + 1 entries, matches one list per edge".into()));
        }
        let (n_images, n_edges) = (image_offsets.len() - 1, edges.len());
        if n_edges == 0 { return Ok((vec![0], Vec::new(), Vec::new(), Vec::new())); }
        let rows = |m: u32| -> usize {
            let m = m as usize;
            if m >= n_images { return 0; }
            let (lo, hi) = ((image_offsets[m] as usize).min(n_rows), (image_offsets[m + 1] as usize).min(n_rows));
            hi.max(lo) - lo
        };
        let (ea, eb): (Vec<u32>, Vec<u32>) = edges.iter().copied().unzip();
        // the a side's edge layout and the match array in it, as build_tracks makes them
        let mut layout = vec![0u64; n_edges + 1];
        for e in 0..n_edges { layout[e + 1] = layout[e] + rows(ea[e]) as u64; }
        let cap = layout[n_edges] as usize;
        let mut m = vec![-1i32; cap];
        for (e, list) in matches.iter().enumerate() {
            for &(i, j) in list {
                if i < rows(ea[e]) { m[layout[e] as usize + i] = j as i32; }
            }
        }
        let mut counts = [0u32; 4];
        let (mut offsets, mut link_a, mut link_b, mut edge_links) = (vec![0u64; n_edges + 1], vec![0i32; cap], vec![0i32; cap], vec![0u32; n_edges]);
        // SAFETY: device buffers sized as declared; n_rows, cap and n_edges bound what is read and written
        unsafe {
            let d_io = DeviceBuffer::from_slice(image_offsets)?;
            let (d_ea, d_eb) = (DeviceBuffer::from_slice(&ea)?, DeviceBuffer::from_slice(&eb)?);
            let d_la = DeviceBuffer::from_slice(&layout)?;
            let d_m = DeviceBuffer::from_slice(&m)?;
            let d_off = DeviceBuffer::<u64>::new(n_edges + 1)?;
            let (d_a, d_b) = (DeviceBuffer::<i32>::new(cap.max(1))?, DeviceBuffer::<i32>::new(cap.max(1))?);
            let d_links = DeviceBuffer::<u32>::new(n_edges)?;
            let d_counts = DeviceBuffer::<u32>::new(4)?;
            check(self.h, ffi::lf_mkd_link_table_device(
                self.h, d_io.as_ptr(), n_images as u32, n_rows as u64, d_ea.as_ptr(), d_eb.as_ptr(), d_la.as_ptr(), cap as u64,
                n_edges as u32, d_m.as_ptr(), min_links, if local { LINK_TABLE_LOCAL } else { 0 }, cap as u64, d_off.as_mut_ptr(),
                d_a.as_mut_ptr(), d_b.as_mut_ptr(), std::ptr::null_mut(), d_links.as_mut_ptr(), std::ptr::null_mut(),
                d_counts.as_mut_ptr(), std::ptr::null_mut()))?;
            check(self.h, ffi::lf_mkd_synchronize(self.h))?;
            d_counts.download(&mut counts)?;
            d_off.download(&mut offsets)?;
            d_links.download(&mut edge_links)?;
            if cap > 0 {
                d_a.download(&mut link_a)?;
                d_b.download(&mut link_b)?;
            }
        }
        link_a.truncate(counts[1] as usize);
        link_b.truncate(counts[1] as usize);
        Ok((offsets, link_a, link_b, edge_links))
    }

    /// The candidate edges of a vote table (`lf_mkd_select_edges_device`): `votes` is `[n_a][n_b]` row-major; per row the `k`
    /// columns with the most votes among those with at least `min_votes` (larger votes first, among equal votes the LOWER
    /// column), `flags` of `SELECT_SKIP_SELF` / `SELECT_UNIQUE`.  Returns (edges, edge_votes, rank): the edges in the order
    /// row, then rank -- with `SELECT_UNIQUE` every unordered pair once, as (smaller, larger) --, the votes of the pick that
    /// made each, and the `[n_a][k]` picks of every row, -1 behind them.
    pub fn select_edges(&mut self, votes: &[u32], n_a: usize, n_b: usize, k: u32, min_votes: u32, flags: u32)
                        -> Result<(Vec<(u32, u32)>, Vec<u32>, Vec<i32>), Error> {
        if votes.len() != n_a * n_b || k == 0 || k > SELECT_MAX_K {
            return Err(Error::BadArgument("select_edges: votes needs n_a * n_b entries, k must be in 1 ..= 32".into()));
        }
        let slots = n_a * k as usize;
        if slots == 0 { return Ok((Vec::new(), Vec::new(), Vec::new())); }
        let mut counts = [0u32; 4];
        let (mut ea, mut eb, mut ev, mut rank) = (vec![0u32; slots], vec![0u32; slots], vec![0u32; slots], vec![0i32; slots]);
        // SAFETY: device buffers sized as declared; n_a, n_b, k and the capacity bound what is read and written
        unsafe {
            let d_votes = DeviceBuffer::from_slice(votes)?;
            let (d_ea, d_eb, d_ev) = (DeviceBuffer::<u32>::new(slots)?, DeviceBuffer::<u32>::new(slots)?, DeviceBuffer::<u32>::new(slots)?);
            let d_rank = DeviceBuffer::<i32>::new(slots)?;
            let d_counts = DeviceBuffer::<u32>::new(4)?;
            check(self.h, ffi::lf_mkd_select_edges_device(
                self.h, d_votes.as_ptr(), n_a as u32, n_b as u32, k, min_votes, flags, slots as u64, d_rank.as_mut_ptr(),
                std::ptr::null_mut(), d_ea.as_mut_ptr(), d_eb.as_mut_ptr(), d_ev.as_mut_ptr(), d_counts.as_mut_ptr(),
                std::ptr::null_mut()))?;
            check(self.h, ffi::lf_mkd_synchronize(self.h))?;
            d_counts.download(&mut counts)?;
            d_ea.download(&mut ea)?;
            d_eb.download(&mut eb)?;
            d_ev.download(&mut ev)?;
            d_rank.download(&mut rank)?;
        }
        let kept = counts[0] as usize;
        ev.truncate(kept);
        Ok((ea.into_iter().zip(eb).take(kept).collect(), ev, rank))
    }

    /// `match_q8_batch` once more under each pair's verified model (`lf_mkd_match_q8_guided_pairs_device`): a row's candidates
    /// are the rows of the other side that pass the verifier's inlier test with it under `models[p]` (row-major H or F, as the
    /// verifiers return it; `kind`: `GUIDE_HOMOGRAPHY` / `GUIDE_FUNDAMENTAL`) within `threshold_px`.  `kps_a` / `kps_b` are
    /// indexed like the descriptor rows.  Lowe's ratio 0.8, both directions, kept only where they agree.  Returns, per pair,
    /// the (row of the pair's a rows, row of its b rows) matches; with the verifier's model, kind and threshold every
    /// verified match is among them.
    pub fn match_q8_guided_batch(&mut self, a: &ArrayView2<u8>, kps_a: &[Keypoint], offsets_a: &[u64], b: &ArrayView2<u8>,
                                 kps_b: &[Keypoint], offsets_b: &[u64], models: &[[f32; 9]], kind: u32, threshold_px: f32)
        -> Result<Vec<Vec<(usize, usize)>>, Error> {
        assert_eq!(a.ncols(), DESCRIPTOR_LEN);
        assert_eq!(b.ncols(), DESCRIPTOR_LEN);
        if offsets_a.is_empty() || offsets_a.len() != offsets_b.len() || models.len() + 1 != offsets_a.len() {
            return Err(Error::BadArgument("match_q8_guided_batch: n_pairs + 1 offsets on either side, one model per pair".into()));
        }
        if kps_a.len() != a.nrows() || kps_b.len() != b.nrows() {
            return Err(Error::BadArgument("match_q8_guided_batch: one keypoint per descriptor row on either side".into()));
        }
        let n_pairs = models.len();
        let (a, b) = (a.as_standard_layout(), b.as_standard_layout());
        let (na, nb) = (a.nrows(), b.nrows());
        let mut m = vec![-1i32; na];
        if n_pairs > 0 && na > 0 && nb > 0 {
            let (ka, kb): (Vec<ffi::lf_mkd_keypoint>, Vec<ffi::lf_mkd_keypoint>) =
                (kps_a.iter().map(from_keypoint).collect(), kps_b.iter().map(from_keypoint).collect());
            let flat: Vec<f32> = models.iter().flatten().copied().collect();
            // SAFETY: a, b are contiguous [n][128]; device buffers sized as declared; `m` has na entries
            unsafe {
                let (d_a, d_b) = (DeviceBuffer::from_slice(a.as_slice().unwrap())?, DeviceBuffer::from_slice(b.as_slice().unwrap())?);
                let (d_ka, d_kb) = (DeviceBuffer::from_slice(&ka)?, DeviceBuffer::from_slice(&kb)?);
                let (d_oa, d_ob) = (DeviceBuffer::from_slice(offsets_a)?, DeviceBuffer::from_slice(offsets_b)?);
                let d_model = DeviceBuffer::from_slice(&flat)?;
                let d_ab = DeviceBuffer::from_slice(&m)?;                    // rows outside every pair stay -1
                let d_ba = DeviceBuffer::<i32>::new(nb)?;
                check(self.h, ffi::lf_mkd_match_q8_guided_pairs_device(
                    self.h, d_a.as_ptr(), d_ka.as_ptr(), d_oa.as_ptr(), na as u64, d_b.as_ptr(), d_kb.as_ptr(), d_ob.as_ptr(),
                    nb as u64, d_model.as_ptr(), n_pairs as u32, kind, threshold_px, 0.8, MATCH_MUTUAL, d_ab.as_mut_ptr(),
                    d_ba.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut()))?;
                check(self.h, ffi::lf_mkd_synchronize(self.h))?;
                d_ab.download(&mut m)?;
            }
        }
        Ok((0..n_pairs).map(|p| {
            let (lo, hi) = ((offsets_a[p] as usize).min(na), (offsets_a[p + 1] as usize).min(na));
            (lo..hi.max(lo)).filter(|&i| m[i] >= 0).map(|i| (i - lo, m[i] as usize)).collect()
        }).collect())
    }

    /// RANSAC fundamental-matrix verification of matches (`lf_mkd_verify_fundamental`, `include/lf_mkd.h` states the
    /// algorithm): 7-point samples scored by Sampson distance on the GPU, then a rank-2 least-squares refit.  `matches` are
    /// (row of `kps_a`, row of `kps_b`) pairs as `match_features` returns them.  Returns F (row-major, b^T F a = 0 in pixels,
    /// its largest entry +1) and the matches within `threshold_px` of Sampson distance; `None` if no sample was valid.
    pub fn verify_fundamental(&mut self, kps_a: &[Keypoint], kps_b: &[Keypoint], matches: &[(usize, usize)],
                              threshold_px: f32, n_hypotheses: u32, seed: u32)
        -> Result<(Option<[f32; 9]>, Vec<(usize, usize)>), Error> {
        let mut m = vec![-1i32; kps_a.len()];
        for &(i, j) in matches {
            if i >= kps_a.len() || j >= kps_b.len() {
                return Err(Error::BadArgument("verify_fundamental: match outside the keypoints".into()));
            }
            m[i] = j as i32;
        }
        let mut f = [0f32; 9];
        let mut ver = vec![-1i32; kps_a.len()];
        let mut stats = [0u32; 4];
        // SAFETY: Keypoint and lf_mkd_keypoint share their layout (asserted above); every array has the length passed
        unsafe {
            check(self.h, ffi::lf_mkd_verify_fundamental(self.h, kps_a.as_ptr() as *const ffi::lf_mkd_keypoint,
                                                         kps_a.len() as u64, kps_b.as_ptr() as *const ffi::lf_mkd_keypoint,
                                                         kps_b.len() as u64, m.as_ptr(), n_hypotheses, threshold_px, seed, 0,
                                                         f.as_mut_ptr(), ver.as_mut_ptr(), stats.as_mut_ptr()))?;
        }
        let inliers = ver.iter().enumerate().filter(|(_, j)| **j >= 0).map(|(i, j)| (i, *j as usize)).collect();
        Ok((if stats[2] == u32::MAX { None } else { Some(f) }, inliers))
    }

    /// The match stage of a job sharded by image over the GPUs of a node (one process and one `LocalFeaturesHip` per GPU;
    /// BASELINE configs[3]): `desc_local` holds this rank's descriptors, image after image (`image_sizes` rows each);
    /// the shards are all-gathered over RCCL -- the path's one collective -- and every local descriptor is matched against
    /// the descriptors of all OTHER images (`match_features`' rule, ratio 0.8).  Returns (local row, global row) pairs;
    /// global rows count through the ranks' shards in rank order.  `comm`: see `HipComm::new`.
    pub fn cross_image_match(&mut self, comm: &HipComm, desc_local: &ArrayView2<f32>, image_sizes: &[usize])
        -> Result<Vec<(usize, usize)>, Error>
    {
        assert_eq!(desc_local.ncols(), DESCRIPTOR_LEN);
        assert_eq!(image_sizes.iter().sum::<usize>(), desc_local.nrows());
        let local = desc_local.as_standard_layout();
        let counts = comm.shard_counts(local.nrows() as u64)?;           // one u64 per rank, exchanged by the application
        let base: u64 = counts[..comm.rank as usize].iter().sum();
        let total: u64 = counts.iter().sum();
        let (mut lo, mut hi) = (Vec::with_capacity(local.nrows()), Vec::with_capacity(local.nrows()));
        let mut start = base as u32;
        for &n in image_sizes {
            for _ in 0..n { lo.push(start); hi.push(start + n as u32); }
            start += n as u32;
        }
        let mut matches = vec![-1i32; local.nrows()];
        // SAFETY: device buffers sized as declared; every rank makes the same collective call
        unsafe {
            let gathered = DeviceBuffer::<f32>::new(total as usize * DESCRIPTOR_LEN)?;
            let own = gathered.as_mut_ptr().add(base as usize * DESCRIPTOR_LEN);
            gathered.upload_at(own, local.as_slice().unwrap())?;
            check(self.h, ffi::lf_mkd_allgather_descriptors(self.h, comm.c, counts.as_ptr(), gathered.as_mut_ptr(),
                                                            ffi::LF_MKD_GATHER_DIRECT, std::ptr::null_mut()))?;
            let (d_lo, d_hi) = (DeviceBuffer::from_slice(&lo)?, DeviceBuffer::from_slice(&hi)?);
            let d_match = DeviceBuffer::<i32>::new(local.nrows())?;
            check(self.h, ffi::lf_mkd_match_device(self.h, own, local.nrows() as u64, gathered.as_mut_ptr(), total,
                                                   d_lo.as_ptr(), d_hi.as_ptr(), 0.8, d_match.as_mut_ptr(),
                                                   std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut()))?;
            check(self.h, ffi::lf_mkd_synchronize(self.h))?;
            d_match.download(&mut matches)?;
        }
        Ok(matches.iter().enumerate().filter(|(_, j)| **j >= 0).map(|(i, j)| (i, *j as usize)).collect())
    }

    fn image_dims(img: &ArrayView2<f32>) -> Result<(u32, u32), Error> {
        let width: u32 = img.ncols().try_into().map_err(|_| Error::BadArgument("image too wide".into()))?;
        let height: u32 = img.nrows().try_into().map_err(|_| Error::BadArgument("image too tall".into()))?;
        Ok((width, height))
    }

    // detect / detect_top_n in one library call: image -> pyramid + a-trous stack -> blobs -> [top n] -> orientation ->
    // sampling -> descriptors, every stage on the device
    fn detect_on_device(&mut self, img: &ArrayView2<f32>, top_n: u32, min_size: f32) -> Result<FeaturesResult, Error> {
        let (width, height) = Self::image_dims(img)?;
        let data = img.as_slice().expect("image must be contiguous row-major"); // vulkan/mod.rs:368
        let cap = self.fixed_params.max_features as usize;
        let mut keypoints = vec![ffi::lf_mkd_keypoint::default(); cap];
        let mut descriptors = Array2::<f32>::zeros((cap, DESCRIPTOR_LEN));
        let (mut n, mut dropped_blobs, mut dropped_features) = (0u64, 0u64, 0u64);
        // SAFETY: `data` holds width*height f32; the two outputs have room for `cap` rows
        unsafe {
            check(self.h, ffi::lf_mkd_detect(self.h, data.as_ptr(), width, height, top_n, min_size, keypoints.as_mut_ptr(),
                                             descriptors.as_mut_ptr(), cap as u64, &mut n, &mut dropped_blobs,
                                             &mut dropped_features))?;
        }
        keypoints.truncate(n as usize);
        Ok(FeaturesResult {
            keypoints: keypoints.into_iter().map(to_keypoint).collect(),
            descriptors: descriptors.slice_move(s![..n as usize, ..]),
            dropped_blobs: dropped_blobs as u32,
            dropped_features: dropped_features as u32,
        })
    }
}

/// One rank's RCCL communicator for `cross_image_match`.  Rank 0 draws the identifier (`HipComm::unique_id`) and hands its
/// 128 bytes to the other ranks by whatever channel the application has; every rank then calls `HipComm::new` with it.
pub struct HipComm {
    c: *mut ffi::lf_mkd_comm,
    pub n_ranks: i32,
    pub rank: i32,
    /// how the application exchanges one u64 per rank (the shard sizes): e.g. over the channel that carried the identifier
    exchange_counts: Box<dyn Fn(u64) -> Vec<u64>>,
}

impl HipComm {
    pub fn unique_id() -> Result<[u8; ffi::LF_MKD_COMM_ID_BYTES], Error> {
        let mut id = [0u8; ffi::LF_MKD_COMM_ID_BYTES];
        // SAFETY: `id` has LF_MKD_COMM_ID_BYTES bytes
        check(std::ptr::null(), unsafe { ffi::lf_mkd_comm_unique_id(id.as_mut_ptr()) })?;
        Ok(id)
    }

    pub fn new(lf: &mut LocalFeaturesHip, id: &[u8; ffi::LF_MKD_COMM_ID_BYTES], n_ranks: i32, rank: i32,
               exchange_counts: Box<dyn Fn(u64) -> Vec<u64>>) -> Result<Self, Error> {
        let mut c = std::ptr::null_mut();
        // SAFETY: collective over the ranks that share `id`
        check(lf.h, unsafe { ffi::lf_mkd_comm_create(lf.h, id.as_ptr(), n_ranks, rank, &mut c) })?;
        Ok(Self { c, n_ranks, rank, exchange_counts })
    }

    fn shard_counts(&self, mine: u64) -> Result<Vec<u64>, Error> {
        let counts = (self.exchange_counts)(mine);
        if counts.len() != self.n_ranks as usize || counts[self.rank as usize] != mine {
            return Err(Error::BadArgument("exchange_counts must return one entry per rank, this rank's own included".into()));
        }
        Ok(counts)
    }

    /// One group of ncclSend + ncclRecv from this rank to itself (`lf_mkd_comm_loopback`): `rows` descriptors go out of one
    /// device buffer and must arrive in another.  What a job runs once per rank before its first `cross_image_match`, so that
    /// the point-to-point branch of the gather has met the machine's librccl before the collective depends on it.
    pub fn self_test(&self, lf: &mut LocalFeaturesHip, rows: usize) -> Result<(), Error> {
        let src: Vec<f32> = (0..rows * DESCRIPTOR_LEN).map(|i| (i % 8191) as f32).collect();
        let mut back = vec![0f32; src.len()];
        // SAFETY: two distinct device buffers of `rows` rows each
        unsafe {
            let (d_src, d_dst) = (DeviceBuffer::from_slice(&src)?, DeviceBuffer::<f32>::new(src.len().max(1))?);
            check(lf.h, ffi::lf_mkd_comm_loopback(lf.h, self.c, d_src.as_ptr(), d_dst.as_mut_ptr(), rows as u64,
                                                  std::ptr::null_mut()))?;
            check(lf.h, ffi::lf_mkd_synchronize(lf.h))?;
            if rows > 0 { d_dst.download(&mut back)?; }
        }
        if back != src { return Err(Error::BadArgument("RCCL loopback: the rows that arrived are not the rows sent".into())); }
        Ok(())
    }

    /// `LF_MKD_GATHER_DIRECT` / `LF_MKD_GATHER_RING` as the latest gather ran, -1 before the first
    pub fn last_form(&self) -> i32 {
        // SAFETY: plain query
        unsafe { ffi::lf_mkd_comm_last_form(self.c) }
    }

    /// (RCCL version code, ranks, this rank)
    pub fn info(&self) -> Result<(i32, i32, i32), Error> {
        let (mut v, mut n, mut r) = (0, 0, 0);
        // SAFETY: plain out-pointers
        check(std::ptr::null(), unsafe { ffi::lf_mkd_comm_info(self.c, &mut v, &mut n, &mut r) })?;
        Ok((v, n, r))
    }
}

impl Drop for HipComm {
    fn drop(&mut self) {
        // SAFETY: `c` came from lf_mkd_comm_create and is destroyed exactly once
        unsafe { ffi::lf_mkd_comm_destroy(self.c); }
    }
}

impl Drop for LocalFeaturesHip {
    fn drop(&mut self) {
        // SAFETY: `h` came from lf_mkd_create* and is destroyed exactly once
        unsafe { ffi::lf_mkd_destroy(self.h) }
    }
}

fn to_keypoint(k: ffi::lf_mkd_keypoint) -> Keypoint {
    Keypoint { x: k.x, y: k.y, size: k.size, angle: k.angle, response: k.response }
}

fn from_keypoint(k: &Keypoint) -> ffi::lf_mkd_keypoint {
    ffi::lf_mkd_keypoint { x: k.x, y: k.y, size: k.size, angle: k.angle, response: k.response }
}
