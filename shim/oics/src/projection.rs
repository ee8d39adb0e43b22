//! `oics::projection` (reference: packages/lib/src/projection.rs:17-194) -> omr_get_angle_with_projections,
//! its batch form omr_get_angles_with_projections_batch, and the batch that also rotates the full-size images,
//! omr_deskew_with_projections_batch.
use crate::bridge::{border_bytes, check, into_mat, view};
use crate::ffi;
use crate::transfer::TransformableMatrix;
use opencv::core::{Mat, Scalar};

/// Scale, gray, threshold, sweep -N..N candidates of `angle_step`, arg-max with the reference's tie policy.
/// `threads` is accepted and ignored: the reference's multi-thread branch rotates by the integer index
/// instead of index * step (projection.rs:94) and no caller uses it.  Panics where the reference panics
/// (`.expect`, projection.rs:26-31,57,61), because the signature has no error channel.
pub fn get_angle_with_projections(
    src: &TransformableMatrix,
    max_angle: u16,
    angle_step: f64,
    resize_scale: f64,
    threads: usize,
) -> f64 {
    let v = view(src.get_mat()).expect("8-bit image");
    let mut angle = 0.0f64;
    let rc = unsafe { ffi::omr_get_angle_with_projections(&v, max_angle, angle_step, resize_scale, threads, &mut angle) };
    if rc != ffi::OMR_OK {
        crate::bridge::check(rc).expect("get_angle_with_projections");
    }
    angle
}

/// `get_angle_with_projections` for a batch: images of any mix of shapes, one angle per image at the image's own
/// position, each the angle the per-call function returns (same f64 bits).  Same-shape images are resized and swept
/// together on the device.  Panics where `get_angle_with_projections` panics; an invalid image fails the whole batch.
pub fn get_angles_with_projections(
    srcs: &[&TransformableMatrix],
    max_angle: u16,
    angle_step: f64,
    resize_scale: f64,
) -> Vec<f64> {
    let views: Vec<ffi::OmrImage> = srcs.iter().map(|s| view(s.get_mat()).expect("8-bit image")).collect();
    let mut angles = vec![0.0f64; srcs.len()];
    let rc = unsafe {
        ffi::omr_get_angles_with_projections_batch(views.as_ptr(), srcs.len() as i32, max_angle, angle_step, resize_scale, angles.as_mut_ptr(), std::ptr::null_mut())
    };
    if rc != ffi::OMR_OK {
        crate::bridge::check(rc).expect("get_angles_with_projections");
    }
    angles
}

/// The reference benchmark's flow (core/src/main.rs:68-95) for a batch -> omr_deskew_with_projections_batch:
/// `get_angle_with_projections(src, max_angle, angle_step, resize_scale, _)` on every image, then
/// `rotate_mat(src, angle, 1.0, flags, BORDER_CONSTANT, border_value, CONTAIN)` of the full-size image.  Images of any mix
/// of shapes; pair i belongs to `srcs[i]`: the per-call angle (same f64 bits) and the rotated image (same bytes).
/// `flags` is INTER_NEAREST (0) or INTER_LINEAR (1); anything else is OMR_ERR_NOTIMPL.
pub fn deskew_with_projections(
    srcs: &[&TransformableMatrix],
    max_angle: u16,
    angle_step: f64,
    resize_scale: f64,
    flags: i32,
    border_value: Scalar,
) -> opencv::Result<Vec<(f64, Mat)>> {
    let mut views = Vec::with_capacity(srcs.len());
    for s in srcs {
        views.push(view(s.get_mat())?);
    }
    let border = border_bytes(border_value);
    let mut angles = vec![0.0f64; srcs.len()];
    let mut outs: Vec<ffi::OmrImageOwned> = (0..srcs.len()).map(|_| ffi::OmrImageOwned::empty()).collect();
    check(unsafe {
        ffi::omr_deskew_with_projections_batch(views.as_ptr(), srcs.len() as i32, max_angle, angle_step, resize_scale, flags, border.as_ptr(), angles.as_mut_ptr(), std::ptr::null_mut(), outs.as_mut_ptr())
    })?;
    // every image is taken over before the first error is reported, so none of the library's buffers is lost
    let mats: Vec<opencv::Result<Mat>> = outs.into_iter().map(into_mat).collect();
    mats.into_iter().zip(angles).map(|(m, a)| Ok((a, m?))).collect()
}
