"""ctypes binding of the C ABI in include/mops_traj.h (libmops_traj.so).

This is the Python side of the drop-in boundary.  There is deliberately no
fallback: if the HIP library is missing the import of any engine entry point
raises, so a GPU box never silently runs something else.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmops_traj.so")

# every symbol include/mops_traj.h declares (checked by tests/test_abi.py)
EXPORTED = (
    "mops_last_error", "mops_abi_version", "mops_selftest_math", "mops_selftest_walk",
    "mops_mesh_create", "mops_mesh_destroy", "mops_mesh_bytes", "mops_mesh_set_edges", "mops_cell_center_velocity_rbf",
    "mops_field_create", "mops_field_create_device", "mops_field_rebuild_device", "mops_field_create_derived", "mops_field_export", "mops_cell_to_vertex_attr",
    "mops_field_destroy", "mops_field_bytes",
    "mops_locate_cells", "mops_locate_cells_hinted", "mops_order_particles", "mops_order_scratch_bytes",
    "mops_order_particles_live", "mops_permute_arrays", "mops_records_clear_dead",
    "mops_traj_num_records", "mops_traj_num_steps", "mops_traj_advance", "mops_traj_finalize", "mops_traj_last_points",
    "mops_layer_velocity_bytes", "mops_field_layer_velocity", "mops_traj_advance_layer", "mops_run_trajectories_layer",
    "mops_traj_alpha_table", "mops_traj_selection",
    "mops_diffusion_scale", "mops_traj_advance_diffuse", "mops_traj_advance_layer_diffuse", "mops_selftest_philox",
    "mops_run_trajectories_diffuse", "mops_run_trajectories_layer_diffuse",
    "mops_traj_sample_attrs", "mops_traj_advance_sampled", "mops_traj_finalize_attrs", "mops_run_pathline_attrs",
    "mops_traj_capture_bytes", "mops_traj_capture_plan", "mops_traj_advance_captured",
    "mops_remove_nan_lines", "mops_remove_nan_ragged", "mops_run_trajectories", "mops_build_id",
    "mops_remap_num_images", "mops_remap_tables", "mops_remap_fixed_depth", "mops_remap_fixed_latitude",
    "mops_remap_fixed_layer", "mops_colormap_rgba8", "mops_colormap_image",
    "mops_section_points", "mops_remap_section", "mops_section_transport",
    "mops_velocity_gradient", "mops_cell_to_vertex_signed",
    "mops_cell_area", "mops_eddy_classify", "mops_label_components", "mops_eddy_count", "mops_eddy_table",
    "mops_density_bytes", "mops_density_accumulate", "mops_density_image",
    "mops_flowmap_lattice", "mops_ftle_image",
    "mops_level_mean", "mops_path_integral_abs", "mops_path_integral_image",
    # include/mops_io.h
    "mops_lines_geo", "mops_write_lines_vtp", "mops_write_lines_txt", "mops_write_pathline_binary",
    "mops_write_png_rgba8", "mops_write_images_vti", "mops_write_image_vti",
    # include/mops_netcdf.h
    "mops_nc_open", "mops_nc_close", "mops_nc_dim_len", "mops_nc_var_info", "mops_nc_read_f64", "mops_nc_read_i64",
    "mops_nc_read_bytes",
)

MOPS_OK, MOPS_ERR_INVALID, MOPS_ERR_HIP, MOPS_ERR_UNSUPPORTED = 0, -1, -2, -3
MOPS_FORWARD, MOPS_BACKWARD = 0, 1
MOPS_RK4, MOPS_EULER = 0, 1
MOPS_RK4_RELOCATE = 2  # pathline RK4 with each stage located in its own cell (the opt-out of quirk Q1; mops_traj.h)
MOPS_LAYER_REFERENCE, MOPS_LAYER_BRACKET = 0, 1
MOPS_DENSITY_COUNT, MOPS_DENSITY_SPEED, MOPS_DENSITY_VALUES = 0, 1, 2
MOPS_MEAN_GROUP = 64  # cells per group of mops_level_mean's sum (include/mops_traj.h: part of the ABI)


class MeshDesc(C.Structure):
    _fields_ = [("n_cells", C.c_int64), ("n_vertices", C.c_int64), ("max_edges", C.c_int32),
                ("n_vert_levels", C.c_int32), ("h_n_edges_on_cell", C.c_void_p),
                ("h_vertices_on_cell", C.c_void_p), ("h_cells_on_cell", C.c_void_p),
                ("h_cells_on_vertex", C.c_void_p), ("h_cell_coord", C.c_void_p), ("h_vertex_coord", C.c_void_p)]


class SnapshotDesc(C.Structure):
    _fields_ = [("timestep", C.c_int32), ("h_layer_thickness", C.c_void_p), ("h_bottom_depth", C.c_void_p),
                ("h_surface_height", C.c_void_p), ("h_zonal_velocity", C.c_void_p),
                ("h_meridional_velocity", C.c_void_p), ("h_vert_velocity_top", C.c_void_p),
                ("h_normal_velocity", C.c_void_p)]


class TrajCfg(C.Structure):
    _fields_ = [("delta_t", C.c_int64), ("simulation_duration", C.c_int64), ("record_t", C.c_int64),
                ("direction", C.c_int32), ("method", C.c_int32)]


class Particles(C.Structure):
    _fields_ = [("n", C.c_int64), ("d_x", C.c_void_p), ("d_y", C.c_void_p), ("d_z", C.c_void_p),
                ("d_depth", C.c_void_p), ("d_cell", C.c_void_p), ("d_death_step", C.c_void_p),
                ("d_order", C.c_void_p), ("d_n_live", C.c_void_p)]


class Diffusion(C.Structure):
    """mops_diffusion: the random walk's diffusivity (m^2/s), Philox seed, epoch word and particle ids."""
    _fields_ = [("kh", C.c_double), ("seed", C.c_uint64), ("epoch", C.c_uint32), ("id_base", C.c_int64),
                ("d_id", C.c_void_p)]


class PermArray(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("d_dst", C.c_void_p), ("elem_bytes", C.c_int64), ("rows", C.c_int64),
                ("row_stride", C.c_int64)]


class RemapCfg(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("min_lat", C.c_double), ("max_lat", C.c_double),
                ("min_lon", C.c_double), ("max_lon", C.c_double), ("fixed_depth", C.c_double),
                ("fixed_latitude", C.c_double), ("min_depth", C.c_double), ("max_depth", C.c_double),
                ("layer_rule", C.c_int32), ("fixed_layer", C.c_double)]


class MopsError(RuntimeError):
    pass


_lib = None


def load(path: str | None = None):
    """Load libmops_traj.so; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("MOPS_TRAJ_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise MopsError(f"HIP engine library not found at {path}: run `python -c \"import __graft_entry__ as g; "
                        f"g.build()\"` (hipcc --offload-arch=gfx950) first")
    # torch ships its own libamdhip64 (SONAME libamdhip64.so.7, but NEEDED as
    # "libamdhip64.so"): load it first so the engine binds to the same HIP
    # runtime instead of pulling a second copy from /opt/rocm -- two runtimes
    # in one process make the second one report "no ROCm-capable device".
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
    st = C.c_int
    lib.mops_last_error.restype = C.c_char_p
    lib.mops_abi_version.restype = I32
    if os.path.abspath(path) == os.path.abspath(LIB_PATH):
        # the product library must be the build of the sources next to it (experiment variants
        # loaded through MOPS_TRAJ_LIB are exempt)
        from . import _build_id
        lib.mops_build_id.restype = C.c_char_p
        have = lib.mops_build_id().decode(errors="replace")
        want = _build_id.MARKER + _build_id.build_id()
        if have != want:
            raise MopsError(f"stale engine library {path}: built as {have!r}, the sources are {want!r}; rebuild with "
                            "`python -c \"import __graft_entry__ as g; g.build()\"`")
    lib.mops_build_id.restype = C.c_char_p
    if hasattr(lib, "mops_selftest_math"):  # (older engine builds timed as variants lack the self-test)
        lib.mops_selftest_math.argtypes = [I64, P, P, I32, P]; lib.mops_selftest_math.restype = st
    if hasattr(lib, "mops_traj_alpha_table"):  # (likewise)
        lib.mops_traj_alpha_table.argtypes = [I64, P]; lib.mops_traj_alpha_table.restype = I64
    if hasattr(lib, "mops_selftest_walk"):
        lib.mops_selftest_walk.argtypes = [P, I64, P, P, P, P]; lib.mops_selftest_walk.restype = st
    if hasattr(lib, "mops_debug_prof_ext"):  # (-DMOPS_PROF experiment builds only: tools/prof_ext.py)
        lib.mops_debug_prof_ext.argtypes = [P, I32]; lib.mops_debug_prof_ext.restype = st
    lib.mops_mesh_create.argtypes = [P, P, P]; lib.mops_mesh_create.restype = st
    lib.mops_mesh_destroy.argtypes = [P]; lib.mops_mesh_destroy.restype = None
    lib.mops_mesh_bytes.argtypes = [P]; lib.mops_mesh_bytes.restype = I64
    lib.mops_mesh_set_edges.argtypes = [P, I64, P, P, P, P]; lib.mops_mesh_set_edges.restype = st
    lib.mops_cell_center_velocity_rbf.argtypes = [P, P, P, P]; lib.mops_cell_center_velocity_rbf.restype = st
    lib.mops_field_create.argtypes = [P, P, P, P]; lib.mops_field_create.restype = st
    lib.mops_field_create_device.argtypes = [P, P, P, P]; lib.mops_field_create_device.restype = st
    lib.mops_field_rebuild_device.argtypes = [P, P, P]; lib.mops_field_rebuild_device.restype = st
    lib.mops_field_create_derived.argtypes = [P, P, P, P, P, P]; lib.mops_field_create_derived.restype = st
    lib.mops_field_export.argtypes = [P, P, P, P, P]; lib.mops_field_export.restype = st
    lib.mops_cell_to_vertex_attr.argtypes = [P, P, P, P]; lib.mops_cell_to_vertex_attr.restype = st
    lib.mops_lines_geo.argtypes = [I64, I64, P, P, P, P]; lib.mops_lines_geo.restype = st
    lib.mops_write_lines_vtp.argtypes = [C.c_char_p, I64, I64, P, P, P, C.c_int]
    lib.mops_write_lines_vtp.restype = st
    lib.mops_write_lines_txt.argtypes = [C.c_char_p, I64, I64, P, P]; lib.mops_write_lines_txt.restype = st
    lib.mops_write_pathline_binary.argtypes = [C.c_char_p, I64, I64, P, P, P, P, C.c_int, C.c_int]
    lib.mops_write_pathline_binary.restype = st
    lib.mops_nc_open.argtypes = [C.c_char_p, P]; lib.mops_nc_open.restype = st
    lib.mops_nc_close.argtypes = [P]; lib.mops_nc_close.restype = None
    lib.mops_nc_dim_len.argtypes = [P, C.c_char_p, P]; lib.mops_nc_dim_len.restype = st
    lib.mops_nc_var_info.argtypes = [P, C.c_char_p, P, P, P, P]; lib.mops_nc_var_info.restype = st
    for fn in ("mops_nc_read_f64", "mops_nc_read_i64", "mops_nc_read_bytes"):
        getattr(lib, fn).argtypes = [P, C.c_char_p, I64, P, I64]
        getattr(lib, fn).restype = st
    lib.mops_field_destroy.argtypes = [P]; lib.mops_field_destroy.restype = None
    lib.mops_field_bytes.argtypes = [P]; lib.mops_field_bytes.restype = I64
    lib.mops_locate_cells.argtypes = [P, I64, P, P, P]; lib.mops_locate_cells.restype = st
    lib.mops_locate_cells_hinted.argtypes = [P, I64, P, P, P, P]; lib.mops_locate_cells_hinted.restype = st
    lib.mops_order_particles.argtypes = [P, I64, P, P, P]; lib.mops_order_particles.restype = st
    lib.mops_traj_num_records.argtypes = [P]; lib.mops_traj_num_records.restype = I64
    lib.mops_traj_num_steps.argtypes = [P]; lib.mops_traj_num_steps.restype = I64
    lib.mops_traj_advance.argtypes = [P, P, P, P, P, I64, I64, P, I64, P]; lib.mops_traj_advance.restype = st
    if hasattr(lib, "mops_traj_selection"):  # (older engine builds timed as variants lack the witness)
        lib.mops_traj_selection.argtypes = [P, P, P, P]; lib.mops_traj_selection.restype = st
    lib.mops_layer_velocity_bytes.argtypes = [P]; lib.mops_layer_velocity_bytes.restype = I64
    lib.mops_field_layer_velocity.argtypes = [P, P, I32, P, P]; lib.mops_field_layer_velocity.restype = st
    lib.mops_traj_advance_layer.argtypes = [P, P, P, P, P, I64, I64, P, I64, P]
    lib.mops_traj_advance_layer.restype = st
    lib.mops_run_trajectories_layer.argtypes = [P, P, P, P, I32, I64, P, P, C.c_float, P, P, P, P, P, P, P, P, P, P]
    lib.mops_run_trajectories_layer.restype = st
    lib.mops_diffusion_scale.argtypes = [C.c_double, I64]; lib.mops_diffusion_scale.restype = C.c_double
    lib.mops_traj_advance_diffuse.argtypes = [P, P, P, P, P, P, I64, I64, P, I64, P]
    lib.mops_traj_advance_diffuse.restype = st
    lib.mops_traj_advance_layer_diffuse.argtypes = [P, P, P, P, P, P, I64, I64, P, I64, P]
    lib.mops_traj_advance_layer_diffuse.restype = st
    lib.mops_selftest_philox.argtypes = [I64, P, P, P, P]; lib.mops_selftest_philox.restype = st
    lib.mops_run_trajectories_diffuse.argtypes = [P, P, P, P, P, I64, P, P, C.c_float, P, P, P, P, P, P, P, P, P, P]
    lib.mops_run_trajectories_diffuse.restype = st
    lib.mops_run_trajectories_layer_diffuse.argtypes = [P, P, P, P, I32, P, I64, P, P, C.c_float, P, P, P, P, P, P, P,
                                                        P, P, P]
    lib.mops_run_trajectories_layer_diffuse.restype = st
    lib.mops_traj_finalize.argtypes = [I64, I64, P, P, I64, I32, P, P, P, P, P, P, P]
    lib.mops_traj_finalize.restype = st
    lib.mops_traj_last_points.argtypes = [I64, I64, P, P, I64, P, P, P]
    lib.mops_traj_last_points.restype = st
    lib.mops_traj_sample_attrs.argtypes = [P, P, P, P, P, I64, I32, P, P, P, I64, P]
    lib.mops_traj_sample_attrs.restype = st
    lib.mops_traj_advance_sampled.argtypes = [P, P, P, P, P, I64, I64, P, I64, I32, P, P, P, I64, P]
    lib.mops_traj_advance_sampled.restype = st
    lib.mops_traj_capture_bytes.argtypes = [I64, I64]; lib.mops_traj_capture_bytes.restype = I64
    lib.mops_traj_capture_plan.argtypes = [P, I64, I64, I64, P, I64]; lib.mops_traj_capture_plan.restype = I64
    lib.mops_traj_advance_captured.argtypes = [P, P, P, P, P, I64, I64, P, I64, I32, P, P, P, I64, P, I64, P]
    lib.mops_traj_advance_captured.restype = st
    lib.mops_traj_finalize_attrs.argtypes = [I64, I64, P, P, I64, I32, P, I64, P, P, P]
    lib.mops_traj_finalize_attrs.restype = st
    lib.mops_run_pathline_attrs.argtypes = [P, P, P, P, I64, P, P, C.c_float, P, P, P, P, P, P, P, P, P, I32, P, P, P,
                                            P]
    lib.mops_run_pathline_attrs.restype = st
    lib.mops_remove_nan_lines.argtypes = [I64, I64, P, P, P, P, P, P]; lib.mops_remove_nan_lines.restype = st
    lib.mops_remove_nan_ragged.argtypes = [I64, P, P, P, P, P, P, P]; lib.mops_remove_nan_ragged.restype = st
    lib.mops_order_scratch_bytes.argtypes = [I64]; lib.mops_order_scratch_bytes.restype = I64
    lib.mops_permute_arrays.argtypes = [I64, P, I32, P, P]; lib.mops_permute_arrays.restype = st
    lib.mops_order_particles_live.argtypes = [P, I64, P, P, P, P, P, I64, P]
    lib.mops_order_particles_live.restype = st
    lib.mops_records_clear_dead.argtypes = [I64, P, I64, I64, P, I64, P]
    lib.mops_records_clear_dead.restype = st
    lib.mops_run_trajectories.argtypes = [P, P, P, P, I64, P, P, C.c_float, P, P, P, P, P, P, P, P, P, P]
    lib.mops_run_trajectories.restype = st
    lib.mops_remap_num_images.argtypes = [I32]; lib.mops_remap_num_images.restype = I32
    lib.mops_remap_tables.argtypes = [P, I32, P, P, P, P]; lib.mops_remap_tables.restype = st
    lib.mops_remap_fixed_depth.argtypes = [P, P, P, I32, P, P, P, P, P, P]; lib.mops_remap_fixed_depth.restype = st
    lib.mops_remap_fixed_latitude.argtypes = [P, P, P, P, P, P]; lib.mops_remap_fixed_latitude.restype = st
    lib.mops_remap_fixed_layer.argtypes = [P, P, P, P, P, P]; lib.mops_remap_fixed_layer.restype = st
    if hasattr(lib, "mops_remap_section"):  # (older engine builds timed as variants lack the sections)
        D = C.c_double
        lib.mops_section_points.argtypes = [I32, P, I32, P, P, P]; lib.mops_section_points.restype = st
        lib.mops_remap_section.argtypes = [P, P, I32, I32, D, D, P, P, I32, P, P, P, P, P, P]
        lib.mops_remap_section.restype = st
        lib.mops_section_transport.argtypes = [I32, I32, P, P, D, D, P, P]; lib.mops_section_transport.restype = st
    if hasattr(lib, "mops_velocity_gradient"):  # (older engine builds timed as variants lack the eddy fields)
        lib.mops_velocity_gradient.argtypes = [P, P, P, P, P, P, P]; lib.mops_velocity_gradient.restype = st
        lib.mops_cell_to_vertex_signed.argtypes = [P, P, P, P]; lib.mops_cell_to_vertex_signed.restype = st
    if hasattr(lib, "mops_label_components"):  # (older engine builds timed as variants lack the eddy census)
        lib.mops_cell_area.argtypes = [P, P, P]; lib.mops_cell_area.restype = st
        lib.mops_eddy_classify.argtypes = [P, P, P, I32, C.c_double, P, P]; lib.mops_eddy_classify.restype = st
        lib.mops_label_components.argtypes = [P, P, P, P, P]; lib.mops_label_components.restype = st
        lib.mops_eddy_count.argtypes = [P, P, I32, P, P, P]; lib.mops_eddy_count.restype = st
        lib.mops_eddy_table.argtypes = [P, P, I64, P, P, P, P, I32, P, P, P, P, P, P, P, P, P]
        lib.mops_eddy_table.restype = st
    lib.mops_colormap_rgba8.argtypes = [P, I32, I32, I32, P, P, P]; lib.mops_colormap_rgba8.restype = st
    lib.mops_colormap_image.argtypes = [P, I32, I32, I32, P, P, P]; lib.mops_colormap_image.restype = st
    lib.mops_density_bytes.argtypes = [I32, I32]; lib.mops_density_bytes.restype = I64
    lib.mops_density_accumulate.argtypes = [P, I64, I64, I64, P, I64, I64, I64, P, I32, P, I64, I64, P, P]
    lib.mops_density_accumulate.restype = st
    lib.mops_density_image.argtypes = [P, P, I32, P, P]; lib.mops_density_image.restype = st
    lib.mops_flowmap_lattice.argtypes = [P, P, P]; lib.mops_flowmap_lattice.restype = st
    lib.mops_ftle_image.argtypes = [P, P, P, P, C.c_double, I32, P, P]; lib.mops_ftle_image.restype = st
    if hasattr(lib, "mops_level_mean"):  # (older engine builds timed as variants lack the path integrals)
        lib.mops_level_mean.argtypes = [I64, I32, P, P, P, P, P]; lib.mops_level_mean.restype = st
        lib.mops_path_integral_abs.argtypes = [I64, I64, I64, P, I64, I64, P, C.c_double, P, P]
        lib.mops_path_integral_abs.restype = st
        lib.mops_path_integral_image.argtypes = [I64, P, P, C.c_double, P, P]
        lib.mops_path_integral_image.restype = st
    lib.mops_write_png_rgba8.argtypes = [C.c_char_p, I32, I32, P]; lib.mops_write_png_rgba8.restype = st
    lib.mops_write_images_vti.argtypes = [C.c_char_p, I32, I32, I32, P, P, P, P, I32]
    lib.mops_write_images_vti.restype = st
    lib.mops_write_image_vti.argtypes = [C.c_char_p, I32, I32, P, P, P]; lib.mops_write_image_vti.restype = st
    _lib = lib
    return lib


def check(status: int, what: str = ""):
    if status != MOPS_OK:
        msg = load().mops_last_error().decode(errors="replace")
        raise MopsError(f"{what} failed (status {status}): {msg}")
