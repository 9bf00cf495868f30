"""segment_tomogram_core (reference: saber/entry_points/inference_core.py:9-98) - the function both `saber segment tomograms` front ends call
per copick run: read the tomogram, run the segmenter, smooth the label volume (per-label adaptive 3-D Gaussian, on the device here), cast
to uint8, write the segmentation, reset the segmenter's inference state.

The copick project layer is NOT re-implemented: the reference reads and writes tomograms through third-party `copick_utils`
(`readers.tomogram`, `writers.segmentation`), which is absent from this image.  The two callables are therefore parameters (defaulting to
copick_utils' own when it is installed), so a maintainer keeps the reference's I/O and swaps only the compute.

segment_micrograph_core (inference_core.py:100-164) - the per-file body of `saber segment micrographs`: read the micrograph (MRC / TIFF),
Fourier-crop to the target resolution, run the 2-D segmenter, write image + label stack as one run of the OME-Zarr store (SURVEY.md 8
row f-4: saber_amd.utils.{mrc,tiff,zarr_v2,zarr_writer}).

refine_membranes_core (reference: saber/entry_points/run_membrane_refinement.py:92-130, run_refinement + return_write_user_id) - the per-run
body of `saber analysis refine-membranes`: read the organelle and the membrane segmentation, refine them on the device
(saber_amd.analysis.OrganelleMembraneFilter.run_labels: the flattened label maps, without the reference's 4-D detour), write the membrane
map and then the organelle map under the `-refined` user ids.

organelle_statistics_core / process_organelles_core (reference: saber/entry_points/run_analysis.py:124-156 process_single_run, :35-122
process_organelles, :185-192 pickable_object_check) - the bodies of `saber analysis save coordinates` / `save statistics`: read the organelle
segmentation of each run, gather the per-label table on the device (saber_amd.analysis.extract_organelle_statistics), save one pick per
organelle and write the size statistics as CSV.  The runs are processed one after another on the device; the reference's process pool, the
copick project layer and the slurm command are not re-implemented."""
import csv
import logging

import numpy as np
import torch

from saber_amd.filters import masks as mask_filters


def _copick_io():
    try:
        from copick_utils.io import readers, writers          # the reference's own I/O layer (inference_core.py:5)
    except ImportError as ex:
        raise ImportError("copick_utils is not installed: pass read_tomogram= / write_segmentation= callables "
                          "(signatures of copick_utils.io.readers.tomogram / writers.segmentation)") from ex
    return readers.tomogram, writers.segmentation


def segment_tomogram_core(run, voxel_size: float, tomogram_algorithm: str, segmentation_name: str, segmentation_session_id: str,
                          slab_thickness: int, num_slabs: int, delta_z: int, display_segmentation: bool, segmenter, gpu_id: int = 0,
                          target_class: int = 1, *, read_tomogram=None, write_segmentation=None, device_prep: bool = False):
    """device_prep: upload the tomogram once and let the segmenter prepare it on the device (smoothing, normalisation, projection:
    saber_amd/utils/volprep.py); False keeps the host preparation of the reference."""
    logger = logging.getLogger(__name__)
    if read_tomogram is None or write_segmentation is None:
        rd, wr = _copick_io()
        read_tomogram, write_segmentation = read_tomogram or rd, write_segmentation or wr
    vol = read_tomogram(run, voxel_size, algorithm=tomogram_algorithm)
    if vol is None:
        logger.info(f"No Tomogram Found for {run.name}")
        return None
    torch.cuda.set_device(gpu_id)
    img_name = run.name + "-" + segmentation_session_id
    if device_prep:
        from saber_amd.utils.volprep import to_device_volume
        vol = to_device_volume(vol, torch.device("cuda", gpu_id))
    if num_slabs > 1:
        segment_mask = segmenter.segment(vol, slab_thickness, num_slabs, delta_z, img_name, display_segmentation)
    else:
        segment_mask = segmenter.segment(vol, slab_thickness, target_class=target_class, save_run=img_name, display=display_segmentation)
    if segment_mask is None:
        logger.info(f"No Segmentation Found for {run.name}")
        return None
    if not display_segmentation:
        segment_mask = mask_filters.fast_3d_gaussian_smoothing(segment_mask, scale=0.05, deviceID=gpu_id)
        segment_mask = segment_mask.astype(np.uint8)
        write_segmentation(run, segment_mask, "saber", name=segmentation_name, session_id=segmentation_session_id, voxel_size=float(voxel_size))
        logger.info(f"Saved Segmentation for {run.name} as {segmentation_name}")
    del vol, segment_mask
    torch.cuda.empty_cache()
    segmenter.inference_state = None
    return


def segment_micrograph_core(input: str, output: str, scale_factor: float, target_resolution: float, display_image: bool,
                            use_sliding_window: bool, gpu_id, models, device_windows: bool = False):
    """device_windows: with use_sliding_window, keep the window masks on the device (saber2D.segment_windows_device) and write the label
    stack from WindowMasks.to_array_host(): no per-mask full-frame bool array is made on the host.  segmenter.masks then holds the
    records without `segmentation`, segmenter.window_masks the device result.  The stored datasets are those of the host route."""
    import os

    from saber_amd.filters.downsample import FourierRescale2D
    from saber_amd.utils import io, zarr_writer
    segmenter = models["segmenter"]
    zwriter = zarr_writer.get_zarr_writer(output)
    zwriter.set_dict_attr("amg", segmenter.adapter_cfg.amg_cfg.to_dict())
    torch.cuda.set_device(gpu_id)
    image, pixel_size = io.read_micrograph(input)
    image = image.astype(np.float32)
    # (the reference compares target_resolution with a pixel size that may be None for TIFF input and fails there; same here)
    if target_resolution is not None and target_resolution > pixel_size:
        image = FourierRescale2D.run(image, target_resolution / pixel_size)
    elif scale_factor is not None:
        image = FourierRescale2D.run(image, scale_factor)
    if device_windows and use_sliding_window:
        wm = segmenter.segment_windows_device(image)
        segmenter.target_class = models.get("target_class", -1)
        segmenter.image0 = segmenter.image = image
        segmenter.masks, segmenter.window_masks = wm.records, wm
        masks = wm.to_array_host()
    else:
        segmenter.segment(image, target_class=models.get("target_class", -1), display=False, use_sliding_window=use_sliding_window)
        masks = mask_filters.masks_to_array(segmenter.masks)
    if isinstance(pixel_size, np.ndarray):
        pixel_size = pixel_size.item()
    pixel_size = pixel_size / 10 if pixel_size is not None else 1        # Angstrom -> nanometer (inference_core.py:144-148)
    out_image = segmenter.image
    if out_image.ndim == 3:
        out_image = out_image[:, :, 0]
    zwriter.write(run_name=os.path.splitext(os.path.basename(input))[0], image=out_image, masks=masks, pixel_size=pixel_size)


def return_write_user_id(user_id, run=None):
    """run_membrane_refinement.py:126-130"""
    return "saber-refined" if user_id is None else user_id + "-refined"


def refine_membranes_core(run, org_info, mem_info, voxel_size, save_session_id, refiner, read_segmentation=None, write_segmentation=None):
    """org_info / mem_info: (name, user_id, session_id) as the reference's CLI passes them.  read_segmentation / write_segmentation: callables
    with the signatures of copick_utils.io.readers.segmentation / writers.segmentation (the defaults when copick_utils is installed).
    Returns None when a segmentation is missing, else {'organelles', 'membranes'}: the two saved 3-D label maps (numpy, the organelle
    input's dtype; organelle v is saved as v + 1, as the reference saves it)."""
    if read_segmentation is None or write_segmentation is None:
        try:
            from copick_utils.io import readers, writers      # the reference's own I/O layer (run_membrane_refinement.py:94)
        except ImportError as ex:
            raise ImportError("copick_utils is not installed: pass read_segmentation= / write_segmentation= callables "
                              "(signatures of copick_utils.io.readers.segmentation / writers.segmentation)") from ex
        read_segmentation, write_segmentation = read_segmentation or readers.segmentation, write_segmentation or writers.segmentation
    org_seg = read_segmentation(run, voxel_size, org_info[0], session_id=org_info[2], user_id=org_info[1])
    mem_seg = read_segmentation(run, voxel_size, mem_info[0], session_id=mem_info[2], user_id=mem_info[1])
    if org_seg is None:
        print(f"No Organele Segmentation Found for {run.name}")
        return None
    elif mem_seg is None:
        print(f"No Membrane Segmentation Found for {run.name}")
        return None
    org_labels, mem_labels = refiner.run_labels(org_seg, mem_seg)
    out_dtype = org_seg.dtype if isinstance(org_seg, np.ndarray) else torch.empty(0, dtype=org_seg.dtype).numpy().dtype
    signed = {torch.uint16: torch.int16, torch.uint32: torch.int32}
    mem_out = mem_labels.cpu().view(signed.get(mem_labels.dtype, mem_labels.dtype)).numpy().astype(out_dtype)
    org_out = org_labels.cpu().view(signed.get(org_labels.dtype, org_labels.dtype)).numpy().astype(out_dtype)
    write_segmentation(run, mem_out, return_write_user_id(mem_info[1], run), name=mem_info[0], session_id=save_session_id, voxel_size=voxel_size)
    write_segmentation(run, org_out, return_write_user_id(org_info[1], run), name=org_info[0], session_id=save_session_id, voxel_size=voxel_size)
    return {"organelles": org_out, "membranes": mem_out}


def organelle_statistics_core(run, organelle_name, session_id, user_id, voxel_size, save_copick, save_statistics, read_segmentation=None,
                              write_picks=None):
    """run_analysis.py:124-156.  read_segmentation: a callable with the signature of copick_utils.io.readers.segmentation (the default when
    copick_utils is installed); write_picks: see saber_amd.analysis.save_coordinates_to_copick.  Returns the run's CSV rows ([] when the
    segmentation is missing or save_statistics is off)."""
    from saber_amd.analysis import extract_organelle_statistics
    if read_segmentation is None:
        try:
            from copick_utils.io import readers              # the reference's own I/O layer (run_analysis.py:127)
        except ImportError as ex:
            raise ImportError("copick_utils is not installed: pass a read_segmentation= callable "
                              "(signature of copick_utils.io.readers.segmentation)") from ex
        read_segmentation = readers.segmentation
    seg = read_segmentation(run, voxel_size, organelle_name, session_id, user_id)
    if seg is None:
        print(f"{run.name} didn't have any {organelle_name} segmentations present!")
        return []
    csv_rows = extract_organelle_statistics(run, seg, organelle_name, session_id, user_id, voxel_size, save_copick, save_statistics,
                                            write_picks=write_picks)
    return csv_rows if save_statistics and csv_rows else []


def pickable_object_check(pickable_objects, organelle_name):
    """run_analysis.py:185-192.  pickable_objects: a copick root (its .pickable_objects are used) or the list itself."""
    objects = getattr(pickable_objects, "pickable_objects", pickable_objects)
    if not any(obj.name == organelle_name for obj in objects):
        available_names = f"Available pickable object names: {', '.join(obj.name for obj in objects)}"
        raise ValueError(f"Pickable Object {organelle_name} not found in Config!\n{available_names}")


def process_organelles_core(runs, organelle_name, session_id, user_id, voxel_size, save_copick=True, save_statistics=True, output="statistics.csv",
                            *, pickable_objects=None, read_segmentation=None, write_picks=None):
    """run_analysis.py:35-122 without the project layer: `runs` are the run objects.  Writes `output` with the reference's header and appends
    the rows of all runs, in run order, when there are any.  With save_copick the organelle must be among `pickable_objects` (a copick root or
    its list of objects).  Returns all CSV rows."""
    if not save_copick and not save_statistics:
        raise ValueError("At least one of save_copick or save_statistics must be True")
    if save_copick:
        if pickable_objects is None:
            raise ValueError("save_copick needs pickable_objects= (the copick root or its pickable objects) for the pickable-object check")
        pickable_object_check(pickable_objects, organelle_name)
    if save_statistics:
        with open(output, "w", newline="") as csvfile:
            csv.writer(csvfile).writerow(["run_id", "label", "volume_nm3", "diameter_nm"])
    all_csv_rows = []
    for run in runs:
        csv_rows = organelle_statistics_core(run, organelle_name, session_id, user_id, voxel_size, save_copick, save_statistics,
                                             read_segmentation=read_segmentation, write_picks=write_picks)
        if csv_rows:
            all_csv_rows.extend(csv_rows)
    if save_statistics and all_csv_rows:
        with open(output, "a", newline="") as csvfile:
            writer = csv.writer(csvfile)
            for row in all_csv_rows:
                writer.writerow(row)
        print(f"\nStatistics saved to {output}")
    completion_msg = []
    if save_copick:
        completion_msg.append("Coordinate extraction")
    if save_statistics:
        completion_msg.append("Statistics calculation")
    print(f"{' and '.join(completion_msg)} complete!")
    return all_csv_rows
