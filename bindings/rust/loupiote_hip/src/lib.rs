//! Safe layer over `libloupiote_hip.so` with the names and the call shapes of the reference's `crates/lib`
//! (`Device`, `Scene`, `SceneGPU`, `ProbeGPU`, `Renderer`, `BlitMode`, `Error`, `loaders::load_gltf`;
//! reference `crates/lib/src/lib.rs:1-11`).  The wgpu parameters of the reference's signatures (`&wgpu::Device`, `&wgpu::Queue`,
//! `&mut wgpu::CommandEncoder`) have no meaning on a compute-only part and are dropped here; INTEGRATION.md §3 shows the
//! adapters that keep them for `crates/standalone`.  NOT COMPILED in the development image (no Rust toolchain — run `cargo check` where one
//! exists before relying on it): the `ffi` module is generated from `include/lpt.h` (`tools/gen_rust_ffi.py`), this file is written against it by hand.
//!
//! Ownership.  The C library keeps the pointers it is handed (`lpt_renderer_set_resources`, `lpt_renderer_resize`, `lpt_renderer_set_comm`), so the
//! handles here are reference-counted (`Rc`) and whoever uses one holds a clone: a `Renderer` keeps its `Device`, its `SceneGPU`, its `ProbeGPU` and
//! its `Comm` alive, a `SceneGPU` / `ProbeGPU` / `Comm` keeps its `Device` alive — what the reference gets from wgpu's reference-counted bind groups
//! (`renderer.rs:687-725`).  Dropping a scene before its renderer is therefore safe in safe code.  (The C side is defensive as well: destroying a
//! scene, probe or communicator detaches the renderers still bound to it.)
//! Threads.  The handles are raw pointers behind `Rc`: neither `Send` nor `Sync`.  One thread drives a device and everything created from it — the
//! reference drives everything from the winit event-loop thread (`crates/standalone/src/app.rs:259-344`).
pub mod ffi;

use std::ffi::{CStr, CString};
use std::ptr;
use std::rc::Rc;

/// reference `crates/lib/src/errors.rs:2-6` (+ the ABI's own codes)
#[derive(Debug)]
pub enum Error {
    FileNotFound(String),
    TextureToBufferReadFail,
    AccelBuild(String),
    Hip(String),
    Rccl(String),
    InvalidArg(String),
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(ffi::lpt_last_error()).to_string_lossy().into_owned() }
}

fn check(status: i32) -> Result<(), Error> {
    match status {
        ffi::LPT_OK => Ok(()),
        ffi::LPT_ERR_FILE_NOT_FOUND => Err(Error::FileNotFound(last_error())),
        ffi::LPT_ERR_READBACK => Err(Error::TextureToBufferReadFail),
        ffi::LPT_ERR_ACCEL_BUILD => Err(Error::AccelBuild(last_error())),
        ffi::LPT_ERR_HIP => Err(Error::Hip(last_error())),
        ffi::LPT_ERR_RCCL => Err(Error::Rccl(last_error())),
        _ => Err(Error::InvalidArg(last_error())),
    }
}

/// reference `crates/lib/src/device.rs:80` `Device::new`: one GPU.  A cheap handle: clones share the device, the last one destroys it
#[derive(Clone)]
pub struct Device { inner: Rc<DeviceInner> }
struct DeviceInner { h: *mut ffi::lpt_device }
impl Drop for DeviceInner { fn drop(&mut self) { unsafe { ffi::lpt_device_destroy(self.h); } } }
impl Device {
    pub fn new(hip_ordinal: i32) -> Result<Self, Error> {
        let mut h = ptr::null_mut();
        check(unsafe { ffi::lpt_device_create(hip_ordinal, &mut h) })?;
        Ok(Self { inner: Rc::new(DeviceInner { h }) })
    }
    fn h(&self) -> *mut ffi::lpt_device { self.inner.h }
    pub fn synchronize(&self) -> Result<(), Error> { check(unsafe { ffi::lpt_device_synchronize(self.h()) }) }
    /// the shading kernels' interface event on the GPU (SPEC.md §21), once per element -> (next direction, weight, kind: 0 reflected / 1 transmitted)
    #[allow(clippy::too_many_arguments)]
    pub fn interface_sample(&self, dirs: &[[f32; 3]], ns: &[[f32; 3]], ngf: &[[f32; 3]], entering: &[u32], base: &[[f32; 3]], ior: &[f32], thin: &[u32],
                            r4: &[f32]) -> Result<(Vec<[f32; 3]>, Vec<[f32; 3]>, Vec<u32>), Error> {
        let n = dirs.len();
        if [ns.len(), ngf.len(), entering.len(), base.len(), ior.len(), thin.len(), r4.len()].iter().any(|&l| l != n) {
            return Err(Error::InvalidArg("interface_sample: the inputs differ in length".into()));
        }
        let (mut wi, mut weight, mut kind) = (vec![[0f32; 3]; n], vec![[0f32; 3]; n], vec![0u32; n]);
        check(unsafe {
            ffi::lpt_interface_sample(self.h(), n as u32, dirs.as_ptr() as *const f32, ns.as_ptr() as *const f32, ngf.as_ptr() as *const f32, entering.as_ptr(),
                                      base.as_ptr() as *const f32, ior.as_ptr(), thin.as_ptr(), r4.as_ptr(), wi.as_mut_ptr() as *mut f32,
                                      weight.as_mut_ptr() as *mut f32, kind.as_mut_ptr())
        })?;
        Ok((wi, weight, kind))
    }
    /// the interface event of a material whose rough bit is set (SPEC.md §29), once per element: rows of {d, Ns, Ngf, entering, base, ior, thin, roughness, r4, u1, u2} ->
    /// (rows of {wi, weight}, kind: 0 reflected / 1 transmitted / 2 ended, + 4 where the smooth event was taken)
    pub fn interface_sample_rough(&self, rows: &[[f32; 19]]) -> Result<(Vec<[f32; 6]>, Vec<u32>), Error> {
        let n = rows.len();
        let (mut out, mut kind) = (vec![[0f32; 6]; n], vec![0u32; n]);
        check(unsafe { ffi::lpt_interface_sample_rough(self.h(), n as u32, rows.as_ptr() as *const f32, out.as_mut_ptr() as *mut f32, kind.as_mut_ptr()) })?;
        Ok((out, kind))
    }
    /// the shading kernels' BSDF on the GPU (SPEC.md §10), once per element: rows of {base, roughness, metallic, N, Ng, V, L, r3, r4, r5} ->
    /// (rows of {pspec, f, pdf, L_s, weight, pdf_s}, ok: 1 where the sample exists)
    pub fn bsdf_probe(&self, rows: &[[f32; 20]]) -> Result<(Vec<[f32; 12]>, Vec<u32>), Error> {
        let n = rows.len();
        let (mut out, mut ok) = (vec![[0f32; 12]; n], vec![0u32; n]);
        check(unsafe { ffi::lpt_bsdf_probe(self.h(), n as u32, rows.as_ptr() as *const f32, out.as_mut_ptr() as *mut f32, ok.as_mut_ptr()) })?;
        Ok((out, ok))
    }
}

/// reference `crates/lib/src/scene.rs:30-54` `Scene` (`Scene::default()` seeds one dummy element per array)
pub struct Scene { h: *mut ffi::lpt_scene }
impl Default for Scene {
    fn default() -> Self {
        let mut h = ptr::null_mut();
        check(unsafe { ffi::lpt_scene_create(&mut h) }).expect("lpt_scene_create");
        Self { h }
    }
}
impl Scene {
    /// `BLASArray::add_bvh_indexed` (reference `loaders/gltf.rs:97-105`): positions are `[f32; 4]`, normals `[f32; 3]`, uvs `[f32; 2]`
    pub fn add_mesh(&mut self, positions: &[[f32; 4]], normals: Option<&[[f32; 3]]>, uvs: Option<&[[f32; 2]]>, indices: Option<&[u32]>) -> Result<u32, Error> {
        let mut out = 0u32;
        let n = positions.len() as u32;
        check(unsafe {
            ffi::lpt_scene_add_mesh(self.h, positions.as_ptr() as *const _, 16,
                                    normals.map_or(ptr::null(), |x| x.as_ptr() as *const _), 12,
                                    uvs.map_or(ptr::null(), |x| x.as_ptr() as *const _), 8, n,
                                    indices.map_or(ptr::null(), |x| x.as_ptr()), indices.map_or(0, |x| x.len() as u32), &mut out)
        })?;
        Ok(out)
    }
    /// `add_instance(blas, transform, material)` (reference `loaders/gltf.rs:141-145`); column-major `glam::Mat4::to_cols_array()`
    pub fn add_instance(&mut self, blas_index: u32, model_to_world: &[f32; 16], material_index: u32) -> Result<u32, Error> {
        let mut out = 0u32;
        check(unsafe { ffi::lpt_scene_add_instance(self.h, blas_index, model_to_world.as_ptr(), material_index, &mut out) })?;
        Ok(out)
    }
    /// `Instance::set_transform` (reference `crates/standalone/src/lib.rs:118-121`)
    pub fn set_instance_transform(&mut self, index: u32, model_to_world: &[f32; 16]) -> Result<(), Error> {
        check(unsafe { ffi::lpt_scene_set_instance_transform(self.h, index, model_to_world.as_ptr()) })
    }
    pub fn add_material(&mut self, material: &ffi::lpt_material) -> Result<u32, Error> {
        let mut out = 0u32;
        check(unsafe { ffi::lpt_scene_add_material(self.h, material, &mut out) })?;
        Ok(out)
    }
    /// SPEC.md §20: alpha-masked (cutout) materials; `mode` is `ffi::LPT_ALPHA_OPAQUE` / `ffi::LPT_ALPHA_MASK`, `alpha_image` an image index or `ffi::LPT_INVALID_INDEX`
    pub fn set_material_alpha(&mut self, material: u32, mode: u32, cutoff: f32, alpha_image: u32) -> Result<(), Error> {
        check(unsafe { ffi::lpt_scene_set_material_alpha(self.h, material, mode, cutoff, alpha_image) })
    }
    /// SPEC.md §26: alpha-blended (stochastic coverage); `material_alpha` then reports `ffi::LPT_ALPHA_BLEND`, `set_material_alpha` with mode 0 or 1 changes it back
    pub fn set_material_alpha_blend(&mut self, material: u32, alpha_image: u32) -> Result<(), Error> {
        check(unsafe { ffi::lpt_scene_set_material_alpha_blend(self.h, material, alpha_image) })
    }
    /// -> (mode, cutoff, alpha_image)
    pub fn material_alpha(&self, material: u32) -> Result<(u32, f32, u32), Error> {
        let (mut mode, mut cutoff, mut image) = (0u32, 0f32, 0u32);
        check(unsafe { ffi::lpt_scene_get_material_alpha(self.h, material, &mut mode, &mut cutoff, &mut image) })?;
        Ok((mode, cutoff, image))
    }
    /// SPEC.md §21: transmissive materials (glass); `factor` 0 = opaque, `thin_walled`: a pane without thickness, else the boundary of a closed solid
    pub fn set_material_transmission(&mut self, material: u32, factor: f32, ior: f32, thin_walled: bool) -> Result<(), Error> {
        check(unsafe { ffi::lpt_scene_set_material_transmission(self.h, material, factor, ior, thin_walled as u32) })
    }
    /// -> (factor, ior, thin_walled)
    pub fn material_transmission(&self, material: u32) -> Result<(f32, f32, bool), Error> {
        let (mut factor, mut ior, mut thin) = (0f32, 0f32, 0u32);
        check(unsafe { ffi::lpt_scene_get_material_transmission(self.h, material, &mut factor, &mut ior, &mut thin) })?;
        Ok((factor, ior, thin != 0))
    }
    /// SPEC.md §29: rough transmission; one bit beside the transmission state, which `set_material_transmission` leaves alone.  It frosts the interface by the material's roughness
    pub fn set_material_transmission_rough(&mut self, material: u32, on: bool) -> Result<(), Error> {
        check(unsafe { ffi::lpt_scene_set_material_transmission_rough(self.h, material, on as u32) })
    }
    pub fn material_transmission_rough(&self, material: u32) -> Result<bool, Error> {
        let mut on = 0u32;
        check(unsafe { ffi::lpt_scene_get_material_transmission_rough(self.h, material, &mut on) })?;
        Ok(on != 0)
    }
    /// SPEC.md §28: volume attenuation (glTF attenuationColor / attenuationDistance) of a solid transmissive material; colour (1, 1, 1) or `f32::INFINITY`: none
    pub fn set_material_attenuation(&mut self, material: u32, color: [f32; 3], distance: f32) -> Result<(), Error> {
        check(unsafe { ffi::lpt_scene_set_material_attenuation(self.h, material, color.as_ptr(), distance) })
    }
    /// -> (color, distance, sigma)
    pub fn material_attenuation(&self, material: u32) -> Result<([f32; 3], f32, [f32; 3]), Error> {
        let (mut color, mut distance, mut sigma) = ([0f32; 3], 0f32, [0f32; 3]);
        check(unsafe { ffi::lpt_scene_get_material_attenuation(self.h, material, color.as_mut_ptr(), &mut distance, sigma.as_mut_ptr()) })?;
        Ok((color, distance, sigma))
    }
    /// SPEC.md §22: emissive materials; `Le = factor x strength` per channel, times the sRGB emissive `image` where one is given; a product of 0: non-emissive again
    pub fn set_material_emission(&mut self, material: u32, factor: [f32; 3], strength: f32, image: Option<u32>) -> Result<(), Error> {
        check(unsafe { ffi::lpt_scene_set_material_emission(self.h, material, factor.as_ptr(), strength, image.unwrap_or(ffi::LPT_INVALID_INDEX)) })
    }
    /// -> (Le, image)
    pub fn material_emission(&self, material: u32) -> Result<([f32; 3], Option<u32>), Error> {
        let (mut le, mut image) = ([0f32; 3], 0u32);
        check(unsafe { ffi::lpt_scene_get_material_emission(self.h, material, le.as_mut_ptr(), &mut image) })?;
        Ok((le, if image == ffi::LPT_INVALID_INDEX { None } else { Some(image) }))
    }
    /// SPEC.md §23 on the host: the emissive triangles' alias table -> (q, alias, prim, prim_alias, sum_w); empty = no distribution
    pub fn emitter_distribution(&self) -> Result<(Vec<f32>, Vec<u32>, Vec<u32>, Vec<u32>, f64), Error> {
        let (mut n, mut total) = (0u32, 0f64);
        check(unsafe { ffi::lpt_scene_emitter_distribution(self.h, 0, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), &mut n, &mut total) })?;
        let cap = n as usize;
        let (mut q, mut alias, mut prim, mut prim_alias) = (vec![0f32; cap], vec![0u32; cap], vec![0u32; cap], vec![0u32; cap]);
        check(unsafe { ffi::lpt_scene_emitter_distribution(self.h, n, q.as_mut_ptr(), alias.as_mut_ptr(), prim.as_mut_ptr(), prim_alias.as_mut_ptr(), &mut n, &mut total) })?;
        Ok((q, alias, prim, prim_alias, total))
    }
    /// SPEC.md §24: a tangent-space normal map; `image = None` removes it
    pub fn set_material_normal_map(&mut self, material: u32, image: Option<u32>, scale: f32) -> Result<(), Error> {
        check(unsafe { ffi::lpt_scene_set_material_normal_map(self.h, material, image.unwrap_or(ffi::LPT_INVALID_INDEX), scale) })
    }
    /// -> (image, scale)
    pub fn material_normal_map(&self, material: u32) -> Result<(Option<u32>, f32), Error> {
        let (mut image, mut scale) = (0u32, 0f32);
        check(unsafe { ffi::lpt_scene_get_material_normal_map(self.h, material, &mut image, &mut scale) })?;
        Ok((if image == ffi::LPT_INVALID_INDEX { None } else { Some(image) }, scale))
    }
    /// SPEC.md §19: a point / spot / directional light (KHR_lights_punctual); records from `punctual_light`
    pub fn add_punctual_light(&mut self, light: &ffi::lpt_punctual_light) -> Result<u32, Error> {
        let mut out = 0u32;
        check(unsafe { ffi::lpt_scene_add_punctual_light(self.h, light, &mut out) })?;
        Ok(out)
    }
    pub fn set_punctual_light(&mut self, index: u32, light: &ffi::lpt_punctual_light) -> Result<(), Error> {
        check(unsafe { ffi::lpt_scene_set_punctual_light(self.h, index, light) })
    }
    pub fn punctual_lights(&self) -> Result<Vec<ffi::lpt_punctual_light>, Error> {
        let mut n = 0u32;
        check(unsafe { ffi::lpt_scene_punctual_count(self.h, &mut n) })?;
        let zero = ffi::lpt_punctual_light { position: [0.0; 4], direction: [0.0; 4], color: [0.0; 4], cone: [0.0; 4] };
        let mut out = vec![zero; n as usize];
        check(unsafe { ffi::lpt_scene_get_punctual_lights(self.h, 0, n, out.as_mut_ptr()) })?;
        Ok(out)
    }
    pub fn add_image(&mut self, rgba8: &[u8], width: u32, height: u32) -> Result<u32, Error> {
        assert!(rgba8.len() >= (width as usize) * (height as usize) * 4);
        let mut out = 0u32;
        check(unsafe { ffi::lpt_scene_add_image(self.h, rgba8.as_ptr(), width, height, &mut out) })?;
        Ok(out)
    }
}
impl Drop for Scene { fn drop(&mut self) { unsafe { ffi::lpt_scene_destroy(self.h); } } }

pub mod loaders {
    use super::{check, ffi, Error, Scene};
    /// reference `crates/lib/src/loaders/gltf.rs:46`: appends to `scene`
    pub fn load_gltf(data: &[u8], scene: &mut Scene) -> Result<(), Error> {
        check(unsafe { ffi::lpt_load_gltf(scene.h, data.as_ptr(), data.len()) })
    }
    /// `flags`: `ffi::LPT_GLTF_READ_BLEND` marks `alphaMode: "BLEND"` materials blended (SPEC.md §26) instead of loading them as opaque;
    /// `ffi::LPT_GLTF_READ_ROUGH_TRANSMISSION` marks transmissive materials rough (SPEC.md §29); 0 is `load_gltf`
    pub fn load_gltf_ex(data: &[u8], scene: &mut Scene, flags: u32) -> Result<(), Error> {
        check(unsafe { ffi::lpt_load_gltf_ex(scene.h, data.as_ptr(), data.len(), flags) })
    }
}

/// reference `crates/lib/src/scene.rs:151` `SceneGPU::new_from_scene` (the CPU scene stays with the caller).  Clones share the device-side scene;
/// a `Renderer` holds one for as long as it is bound to it
#[derive(Clone)]
pub struct SceneGPU { inner: Rc<SceneGpuInner> }
struct SceneGpuInner { h: *mut ffi::lpt_scene_gpu, _device: Device }
impl Drop for SceneGpuInner { fn drop(&mut self) { unsafe { ffi::lpt_scene_gpu_destroy(self.h); } } }
impl SceneGPU {
    pub fn new_from_scene(scene: &Scene, device: &Device) -> Result<Self, Error> {
        let mut h = ptr::null_mut();
        check(unsafe { ffi::lpt_scene_upload(device.h(), scene.h, &mut h) })?;
        Ok(Self { inner: Rc::new(SceneGpuInner { h, _device: device.clone() }) })
    }
    fn h(&self) -> *mut ffi::lpt_scene_gpu { self.inner.h }
    /// after `Scene::set_instance_transform`: re-bake the moved instances and refit the tree on the GPU (the library submits the frames
    /// recorded against the old poses first)
    pub fn update_instances(&self, scene: &Scene) -> Result<u32, Error> {
        let mut n = 0u32;
        check(unsafe { ffi::lpt_scene_gpu_update_instances(self.h(), scene.h, &mut n) })?;
        Ok(n)
    }
    /// after `Scene::set_punctual_light`: the punctual lights to the device again, nothing else (same count; frames recorded against the
    /// old lights are submitted first)
    pub fn update_punctual(&self, scene: &Scene) -> Result<(), Error> {
        check(unsafe { ffi::lpt_scene_gpu_update_punctual(self.h(), scene.h) })
    }
    /// the shading kernels' punctual-light function on the GPU (SPEC.md §19): points -> (direction to the light, distance, incident term)
    pub fn sample_punctual(&self, device: &Device, light: u32, points: &[[f32; 3]]) -> Result<(Vec<[f32; 3]>, Vec<f32>, Vec<[f32; 3]>), Error> {
        let n = points.len();
        let (mut wi, mut dist, mut e) = (vec![[0f32; 3]; n], vec![0f32; n], vec![[0f32; 3]; n]);
        check(unsafe {
            ffi::lpt_scene_gpu_sample_punctual(device.h(), self.h(), light, points.as_ptr() as *const f32, n as u32,
                                               wi.as_mut_ptr() as *mut f32, dist.as_mut_ptr(), e.as_mut_ptr() as *mut f32)
        })?;
        Ok((wi, dist, e))
    }
}

/// SPEC.md §19: the record of a KHR_lights_punctual light (`kind`: `ffi::LPT_PUNCTUAL_POINT` / `_SPOT` / `_DIRECTIONAL`); angles in radians
pub fn punctual_light(kind: u32, position: [f32; 3], direction: [f32; 3], color: [f32; 3], intensity: f32, range: f32, inner_angle: f32,
                      outer_angle: f32) -> Result<ffi::lpt_punctual_light, Error> {
    let mut l = ffi::lpt_punctual_light { position: [0.0; 4], direction: [0.0; 4], color: [0.0; 4], cone: [0.0; 4] };
    check(unsafe {
        ffi::lpt_punctual_light_make(kind, position.as_ptr(), direction.as_ptr(), color.as_ptr(), intensity, range, inner_angle, outer_angle, &mut l)
    })?;
    Ok(l)
}

/// reference `crates/lib/src/scene.rs:72` `ProbeGPU::new`: RGBE8, equirectangular
#[derive(Clone)]
pub struct ProbeGPU { inner: Rc<ProbeInner> }
struct ProbeInner { h: *mut ffi::lpt_probe, _device: Device }
impl Drop for ProbeInner { fn drop(&mut self) { unsafe { ffi::lpt_probe_destroy(self.h); } } }
impl ProbeGPU {
    pub fn new(device: &Device, rgbe8: &[u8], width: u32, height: u32) -> Result<Self, Error> {
        assert!(rgbe8.len() >= (width as usize) * (height as usize) * 4);
        let mut h = ptr::null_mut();
        check(unsafe { ffi::lpt_probe_upload(device.h(), rgbe8.as_ptr(), width, height, &mut h) })?;
        Ok(Self { inner: Rc::new(ProbeInner { h, _device: device.clone() }) })
    }
    fn h(&self) -> *mut ffi::lpt_probe { self.inner.h }
}

/// reference `crates/lib/src/renderer.rs:160-167` (the spelling `Pahtrace` is the reference's)
#[derive(Copy, Clone, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum BlitMode { Pahtrace = 0, DenoisedPathrace = 1, Temporal = 2, GBuffer = 3, MotionVector = 4 }

/// SPEC.md §30: the tone curve of `Renderer::set_display` (`ffi::LPT_DISPLAY_*`)
#[derive(Copy, Clone, Debug, PartialEq, Eq)]
#[repr(u32)]
pub enum DisplayOperator { Clamp = 0, PbrNeutral = 1, Aces = 2 }

/// what `Renderer::meter` returns (SPEC.md §30.3): the suggested exposure, the luminance histogram (384 bins, 8 per octave from 2^-24), the samples the
/// exposure rests on behind the trim, and the sampled pixels without a bin (NaN, infinite, below 2^-24, at or above 2^24)
#[derive(Clone, Debug)]
pub struct Metering { pub ev: f32, pub histogram: Vec<u32>, pub counted: u32, pub skipped: u32 }

/// reference `crates/lib/src/renderer.rs:169-811`
pub struct Renderer {
    h: *mut ffi::lpt_renderer,
    /// pub field of the reference (`renderer.rs:203`); applied by `resize`
    pub downsample_factor: f32,
    /// pub field of the reference (`renderer.rs:204`); handed to the library by `raytrace`
    pub accumulate: bool,
    size: (u32, u32),
    // what the C renderer points at: kept alive here (declared after `h`'s users; `Drop for Renderer` destroys the C renderer first)
    _device: Device,
    scene: Option<SceneGPU>,
    probe: Option<ProbeGPU>,
    comm: Option<Comm>,
}
impl Renderer {
    /// `renderer.rs:209`
    pub fn max_ssbo_element_in_bytes() -> u32 { unsafe { ffi::lpt_max_per_pixel_bytes() } }
    /// `renderer.rs:220` (the swapchain format has no meaning here)
    pub fn new(device: &Device, original_size: (u32, u32)) -> Result<Self, Error> {
        let mut h = ptr::null_mut();
        check(unsafe { ffi::lpt_renderer_create(device.h(), original_size.0, original_size.1, &mut h) })?;
        let mut r = Self { h, downsample_factor: 0.5, accumulate: false, size: (0, 0), _device: device.clone(), scene: None, probe: None, comm: None };
        unsafe { ffi::lpt_renderer_get_size(r.h, &mut r.size.0, &mut r.size.1); }
        Ok(r)
    }
    /// `renderer.rs:326`
    pub fn resize(&mut self, scene: &SceneGPU, probe: Option<&ProbeGPU>, size: (u32, u32)) -> Result<(), Error> {
        check(unsafe { ffi::lpt_renderer_set_downsample(self.h, self.downsample_factor) })?;
        check(unsafe { ffi::lpt_renderer_resize(self.h, scene.h(), probe.map_or(ptr::null(), |p| p.h() as *const _), size.0, size.1) })?;
        self.scene = Some(scene.clone());
        self.probe = probe.cloned();
        check(unsafe { ffi::lpt_renderer_get_size(self.h, &mut self.size.0, &mut self.size.1) })
    }
    /// `renderer.rs:687`
    pub fn set_resources(&mut self, scene: &SceneGPU, probe: Option<&ProbeGPU>) -> Result<(), Error> {
        check(unsafe { ffi::lpt_renderer_set_resources(self.h, scene.h(), probe.map_or(ptr::null(), |p| p.h() as *const _)) })?;
        self.scene = Some(scene.clone());   // the C renderer keeps these pointers: so does this one
        self.probe = probe.cloned();
        Ok(())
    }
    /// `renderer.rs:392`: RECORDS one sample per pixel from `view_transform` (camera-to-world, column-major); launched by the next
    /// submission point (`submit`, any read) — INTEGRATION.md §3a
    pub fn raytrace(&mut self, view_transform: &[f32; 16]) -> Result<(), Error> {
        check(unsafe { ffi::lpt_renderer_set_accumulate(self.h, self.accumulate as i32) })?;
        check(unsafe { ffi::lpt_renderer_raytrace(self.h, view_transform.as_ptr()) })
    }
    /// the app's `queue.submit(Some(encoder.finish()))` (`crates/standalone/src/app.rs:335-337`)
    pub fn submit(&mut self) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_submit(self.h) }) }
    /// `renderer.rs:609`
    pub fn reset_accumulation(&mut self) -> Result<(), Error> {
        self.accumulate = false;
        check(unsafe { ffi::lpt_renderer_reset_accumulation(self.h) })
    }
    /// `renderer.rs:620`
    pub fn upload_noise_texture(&mut self, data: &[u8], width: u32, height: u32, bytes_per_row: u32) -> Result<(), Error> {
        assert!(data.len() >= (bytes_per_row as usize) * (height as usize));
        check(unsafe { ffi::lpt_renderer_upload_noise(self.h, data.as_ptr(), width, height, bytes_per_row) })
    }
    /// `renderer.rs:666`
    pub fn use_noise_texture(&mut self, flag: bool) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_use_noise(self.h, flag as i32) }) }
    /// `renderer.rs:675`
    pub fn set_blit_mode(&mut self, mode: BlitMode) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_set_blit_mode(self.h, mode as i32) }) }
    /// `renderer.rs:683`
    pub fn get_size(&self) -> &(u32, u32) { &self.size }
    /// `renderer.rs:727`: tight rows of sRGB RGBA8; blocking (the reference awaits `device.poll(Wait)`, `:791`)
    pub fn read_pixels(&mut self) -> Result<Vec<u8>, Error> {
        let mut out = vec![0u8; (self.size.0 as usize) * (self.size.1 as usize) * 4];
        check(unsafe { ffi::lpt_renderer_read_pixels(self.h, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// new: the mean radiance as float RGBA (the parity surface)
    pub fn read_radiance(&mut self) -> Result<Vec<f32>, Error> {
        let mut out = vec![0f32; (self.size.0 as usize) * (self.size.1 as usize) * 4];
        check(unsafe { ffi::lpt_renderer_read_radiance(self.h, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// new (multi-GPU, host-side gather): this rank's OWNED pixels of the mean radiance straight into `frame`, a whole-frame buffer in
    /// page-locked host memory (`HostFrame`, or memory passed to `ffi::lpt_host_register` — a shared-memory segment every rank maps);
    /// the other ranks' pixels are left alone.  INTEGRATION.md §9.
    pub fn read_radiance_owned(&mut self, frame: &mut HostFrame) -> Result<(), Error> {
        assert!(frame.len >= (self.size.0 as usize) * (self.size.1 as usize) * 4);
        check(unsafe { ffi::lpt_renderer_read_radiance_owned(self.h, frame.ptr) })
    }
    /// the same into the node's shared frame (`SharedFrame`): every rank writes its own pixels, `SharedFrame::barrier` completes the frame
    pub fn read_radiance_owned_shared(&mut self, frame: &SharedFrame) -> Result<(), Error> {
        assert!(frame.len >= (self.size.0 as usize) * (self.size.1 as usize) * 4);
        check(unsafe { ffi::lpt_renderer_read_radiance_owned(self.h, frame.ptr) })
    }
    /// `renderer.rs:551` without a swapchain: sRGB RGBA8 into the caller's rows
    pub fn blit_rgba8(&mut self, dst: &mut [u8], row_bytes: usize) -> Result<(), Error> {
        assert!(row_bytes >= (self.size.0 as usize) * 4 && dst.len() >= row_bytes * (self.size.1 as usize));
        check(unsafe { ffi::lpt_renderer_blit_rgba8(self.h, dst.as_mut_ptr(), row_bytes) })
    }
    /// build-only knobs (the reference's constants: 3 bounces, `renderer.rs:398-399`)
    pub fn set_max_bounces(&mut self, bounces: u32) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_set_max_bounces(self.h, bounces) }) }
    pub fn set_seed(&mut self, seed: u32) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_set_seed(self.h, seed) }) }
    /// `SPEC.md` §18: next-event estimation samples the environment probe too (off by default; frames change with it)
    pub fn set_env_sampling(&mut self, on: bool) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_set_env_sampling(self.h, on as i32) }) }
    /// SPEC.md §25: a thin-lens camera — lens radius in world units (0, the default: the pinhole) and the distance of the plane in focus; frames change
    /// with it, so `reset_accumulation` belongs after the call
    pub fn set_lens(&mut self, radius: f32, focus_distance: f32) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_set_lens(self.h, radius, focus_distance) }) }
    /// (radius, focus distance)
    pub fn lens(&self) -> Result<(f32, f32), Error> {
        let (mut r, mut f) = (0f32, 0f32);
        check(unsafe { ffi::lpt_renderer_get_lens(self.h, &mut r, &mut f) })?;
        Ok((r, f))
    }
    /// SPEC.md §30: the display transform of `blit` / `read_pixels` — the mean times 2^`exposure_ev`, then the operator's curve, then sRGB; `(0.0, Clamp)`, the
    /// default, is every byte as before.  Nothing is rendered or reset, and the float outputs stay linear
    pub fn set_display(&mut self, exposure_ev: f32, op: DisplayOperator) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_set_display(self.h, exposure_ev, op as u32) }) }
    /// (exposure, operator)
    pub fn display(&self) -> Result<(f32, DisplayOperator), Error> {
        let (mut ev, mut op) = (0f32, 0u32);
        check(unsafe { ffi::lpt_renderer_get_display(self.h, &mut ev, &mut op) })?;
        let op = match op as std::os::raw::c_int {
            ffi::LPT_DISPLAY_PBR_NEUTRAL => DisplayOperator::PbrNeutral,
            ffi::LPT_DISPLAY_ACES => DisplayOperator::Aces,
            _ => DisplayOperator::Clamp,
        };
        Ok((ev, op))
    }
    /// SPEC.md §30.3: the exposure that puts the mean log2 luminance of the presented frame at 18 % grey, without its darkest `low` and brightest `high`
    /// fraction, with the 384-bin histogram it comes from.  `counted == 0`: no sample was left and `ev` is 0.  Nothing is set: pass `ev` to `set_display`
    pub fn meter(&mut self, low: f32, high: f32) -> Result<Metering, Error> {
        let mut m = Metering { ev: 0.0, histogram: vec![0u32; 384], counted: 0, skipped: 0 };
        check(unsafe { ffi::lpt_renderer_meter(self.h, low, high, &mut m.ev, m.histogram.as_mut_ptr(), &mut m.counted, &mut m.skipped) })?;
        Ok(m)
    }
    /// SPEC.md §25, for tests and tools: the primary rays of sample `sample` of the next `raytrace` call, `(origins, dirs)` with 3 floats per pixel of the
    /// full frame (zeros at pixels this rank does not own)
    pub fn primary_rays(&mut self, view_transform: &[f32; 16], sample: u32) -> Result<(Vec<f32>, Vec<f32>), Error> {
        let (mut w, mut h) = (0u32, 0u32);
        check(unsafe { ffi::lpt_renderer_get_size(self.h, &mut w, &mut h) })?;
        let n = 3 * (w as usize) * (h as usize);
        let (mut o, mut d) = (vec![0f32; n], vec![0f32; n]);
        check(unsafe { ffi::lpt_renderer_primary_rays(self.h, view_transform.as_ptr(), sample, o.as_mut_ptr(), d.as_mut_ptr()) })?;
        Ok((o, d))
    }
    /// SPEC.md §23: next-event estimation samples the emissive triangles too; off by default
    pub fn set_emissive_sampling(&mut self, on: bool) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_set_emissive_sampling(self.h, on as i32) }) }
    pub fn emissive_sampling(&self) -> Result<bool, Error> {
        let mut f = 0i32;
        check(unsafe { ffi::lpt_renderer_get_emissive_sampling(self.h, &mut f) })?;
        Ok(f != 0)
    }
    /// SPEC.md §27: punctual lights' shadow rays pass thin-walled transmissive triangles; off by default
    pub fn set_glass_shadows(&mut self, on: bool) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_set_glass_shadows(self.h, on as i32) }) }
    pub fn glass_shadows(&self) -> Result<bool, Error> {
        let mut f = 0i32;
        check(unsafe { ffi::lpt_renderer_get_glass_shadows(self.h, &mut f) })?;
        Ok(f != 0)
    }
    /// launch tuning (the `LPT_OPT_` constants of `ffi`): never changes a frame
    pub fn set_option(&mut self, option: i32, value: u64) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_set_option(self.h, option, value) }) }
    /// tile-sharded frames: bind a communicator (implies `set_shard(rank, world, 32, 8)`), then `exchange` after the frame's `raytrace` calls
    pub fn set_comm(&mut self, comm: &Comm) -> Result<(), Error> {
        check(unsafe { ffi::lpt_renderer_set_comm(self.h, comm.h()) })?;
        self.comm = Some(comm.clone());
        Ok(())
    }
    pub fn exchange(&mut self, mode: i32) -> Result<(), Error> { check(unsafe { ffi::lpt_renderer_exchange(self.h, mode) }) }
}
impl Drop for Renderer { fn drop(&mut self) { unsafe { ffi::lpt_renderer_destroy(self.h); } } }

/// page-locked host memory (`lpt_host_alloc`): a read-back destination the GPU writes by DMA or by zero-copy stores
pub struct HostFrame { ptr: *mut f32, len: usize }
impl HostFrame {
    pub fn new(floats: usize) -> Result<Self, Error> {
        let mut p: *mut std::os::raw::c_void = ptr::null_mut();
        check(unsafe { ffi::lpt_host_alloc(floats * 4, &mut p) })?;
        Ok(Self { ptr: p as *mut f32, len: floats })
    }
    pub fn as_slice(&self) -> &[f32] { unsafe { std::slice::from_raw_parts(self.ptr, self.len) } }
}
impl Drop for HostFrame { fn drop(&mut self) { unsafe { ffi::lpt_host_free(self.ptr as *mut _); } } }

/// the host-side gather of a tile-sharded frame (`lpt_host_frame_*`): ONE whole frame in POSIX shared memory that every rank
/// of a node maps and page-locks.  Per frame: `renderer.read_radiance_owned_shared(&frame)` on every rank, then `frame.barrier(rank, frame_no)`.
pub struct SharedFrame { h: *mut ffi::lpt_host_frame, ptr: *mut f32, len: usize }
impl SharedFrame {
    fn open(name: &str, size: (u32, u32), world: u32, host_only: bool, create: bool) -> Result<Self, Error> {
        let c = CString::new(name).map_err(|_| Error::InvalidArg("name contains a NUL".into()))?;
        let flags = if host_only { ffi::LPT_HOST_FRAME_HOST_ONLY as u32 } else { 0 };
        let mut h = ptr::null_mut();
        check(unsafe {
            if create { ffi::lpt_host_frame_create(c.as_ptr(), size.0, size.1, world, flags, &mut h) } else { ffi::lpt_host_frame_attach(c.as_ptr(), size.0, size.1, world, flags, &mut h) }
        })?;
        let mut p: *mut f32 = ptr::null_mut();
        check(unsafe { ffi::lpt_host_frame_ptr(h, &mut p) })?;
        Ok(Self { h, ptr: p, len: (size.0 as usize) * (size.1 as usize) * 4 })
    }
    /// rank 0; `name` as for `shm_open` ("/something")
    pub fn create(name: &str, size: (u32, u32), world: u32) -> Result<Self, Error> { Self::open(name, size, world, false, true) }
    /// the other ranks, once rank 0 has created it; `host_only`: a participant without a GPU that only reads the finished frame
    pub fn attach(name: &str, size: (u32, u32), world: u32, host_only: bool) -> Result<Self, Error> { Self::open(name, size, world, host_only, false) }
    /// returns when every participant has called it with this frame number (1, 2, 3, ...)
    pub fn barrier(&self, rank: u32, frame_no: u32, timeout_ms: u32) -> Result<(), Error> { check(unsafe { ffi::lpt_host_frame_barrier(self.h, rank, frame_no, timeout_ms) }) }
    /// the frame (complete after `barrier`)
    pub fn as_slice(&self) -> &[f32] { unsafe { std::slice::from_raw_parts(self.ptr, self.len) } }
}
impl Drop for SharedFrame { fn drop(&mut self) { unsafe { ffi::lpt_host_frame_destroy(self.h); } } }

/// one rank of a node-wide frame (new functionality: the reference is single-GPU); RCCL lives inside the library
#[derive(Clone)]
pub struct Comm { inner: Rc<CommInner> }
struct CommInner { h: *mut ffi::lpt_comm, _device: Device }
impl Drop for CommInner { fn drop(&mut self) { unsafe { ffi::lpt_comm_destroy(self.h); } } }
impl Comm {
    fn h(&self) -> *mut ffi::lpt_comm { self.inner.h }
    /// rank 0 creates the id and ships its 128 bytes to the other ranks out of band
    pub fn unique_id() -> Result<[u8; 128], Error> {
        let mut id = [0u8; 128];
        check(unsafe { ffi::lpt_comm_unique_id(id.as_mut_ptr() as *mut _) })?;
        Ok(id)
    }
    pub fn new(device: &Device, unique_id: &[u8; 128], rank: i32, world_size: i32) -> Result<Self, Error> {
        let mut h = ptr::null_mut();
        check(unsafe { ffi::lpt_comm_create(device.h(), unique_id.as_ptr() as *const _, rank, world_size, &mut h) })?;
        Ok(Self { inner: Rc::new(CommInner { h, _device: device.clone() }) })
    }
}
