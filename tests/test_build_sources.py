"""build.SOURCES is kept by hand: every csrc/*.hip file must be listed in it, and every listed file must exist."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sources_list_equals_the_hip_files_of_csrc():
    from unpaired_image_captioning_amd import build
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "unpaired_image_captioning_amd", "csrc", "*.hip")))
    assert len(build.SOURCES) == len(set(build.SOURCES)), "a file is listed twice"
    assert sorted(build.SOURCES) == on_disk, set(build.SOURCES) ^ set(on_disk)
