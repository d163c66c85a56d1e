"""The native library's environment switches (no GPU needed): hcflow_amd/csrc/hcf_switches.h is the one list and the one
reader, INTEGRATION.md repeats exactly that list, every listed switch is run by a test or a tool -- a switch lives only
while something runs it -- and the switches retired for want of that stay gone."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hcflow_amd", "csrc")
HEADER = os.path.join(CSRC, "hcf_switches.h")
BUILT = (".so", ".o", ".a", ".pyc", ".hsaco", ".co")

RETIRED = (
    "HCF_NO_WINO", "HCF_NO_W4F", "HCF_NO_DENSE_WINO", "HCF_NO_WINO_PAD", "HCF_NO_FAT", "HCF_FAT12_PIXELS", "HCF_WINO_MIN_CIN",
    "HCF_WINO_TOP_WAIT", "HCF_NO_N16", "HCF_NO_FCN12", "HCF_NO_FUSE_FCN", "HCF_NO_FUSE_TAIL", "HCF_NO_WGRAD_STREAM",
    "HCF_NO_DG_STREAM", "HCF_NO_WG_BATCH", "HCF_WG_BATCH_BLOCKS", "HCF_NO_DGRAD_WINO", "HCF_WG_BLOCKS", "HCF_WG_DBG", "HCF_EPI_PPB",
)


def files_under(*tops):
    for top in tops:
        for d, dirs, names in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x != "__pycache__"]
            for n in names:
                if not n.endswith(BUILT):
                    yield os.path.join(d, n)


def listed():
    """Names of the X-macro's lines."""
    names = re.findall(r"^\s*X\((HCF_\w+),", open(HEADER).read(), re.M)
    assert names and len(names) == len(set(names))
    return set(names)


def documented():
    """Native HCF_* names of INTEGRATION.md: first column of the table under 'Native switches'."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text.split("### Native switches", 1)[1].split("\n#", 1)[0]
    names = set()
    for line in section.splitlines():
        if line.startswith("| `"):
            names.update(re.findall(r"`(HCF_\w+?)(?:=[^`]*)?`", line.split("|")[1]))
    return names


def test_only_the_switch_header_reads_the_environment():
    for path in files_under(os.path.join("hcflow_amd", "csrc")):
        if path != HEADER:
            assert "getenv" not in open(path, errors="replace").read(), path
    assert "getenv" in open(HEADER).read()


def test_the_document_lists_the_headers_switches():
    assert listed() == documented()
    assert len(listed()) == 14


def test_every_switch_is_run_by_a_test_or_a_tool():
    me = os.path.abspath(__file__)
    text = "\n".join(open(p, errors="replace").read() for p in files_under("tests", "tools") if p != me)
    idle = sorted(n for n in listed() if not re.search(r"\b%s\b" % n, text))
    assert not idle, idle


def test_retired_switches_stay_gone():
    assert len(set(RETIRED)) == 20 and not set(RETIRED) & listed()
    pat = re.compile(r"\b(%s)\b" % "|".join(RETIRED))
    me = os.path.abspath(__file__)
    paths = [p for p in files_under("hcflow_amd", "include", "tests", "tools") if p != me]
    paths += [os.path.join(ROOT, n) for n in ("INTEGRATION.md", "README.md", "DESIGN.md")]
    for path in paths:
        m = pat.search(open(path, errors="replace").read())
        assert m is None, (path, m.group(0))
