//! `oics::projection` (reference: packages/lib/src/projection.rs:17-194) -> omr_get_angle_with_projections,
//! and its batch form omr_get_angles_with_projections_batch.
use crate::bridge::view;
use crate::ffi;
use crate::transfer::TransformableMatrix;

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
