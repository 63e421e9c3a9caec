"""The tools that read kernel names, on the CPU: tools/pmc_summary.py keys a profile's rows by kernel under the names of before and since the form words
(loupiote_amd/csrc/kernel_forms.h), and tools/kernel_bodies.py gives two listings of the same code the same digests."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pmc_summary_keys_old_and_new_names_alike():
    short = _tool("pmc_summary").short
    for name, key in (
            ("void lptd::k_shade<false, false, false, false, false, false, false>(lptd::ShadeKernargs)", "k_shade<false>"),
            ("void lptd::k_shade<true, true, false, false, true, true, false>(lptd::ShadeKernargs)", "k_shade<true>"),
            ("void lptd::k_shade<false>(lptd::ShadeKernargs)", "k_shade<false>"),
            ("void lptd::k_shade<0u>(lptd::ShadeKernargs)", "k_shade<false>"),
            ("void lptd::k_shade<1u>(lptd::ShadeKernargs)", "k_shade<true>"),
            ("void lptd::k_shade<118u>(lptd::ShadeKernargs)", "k_shade<false>"),
            ("void lptd::k_shade<51>(lptd::ShadeKernargs)", "k_shade<true>"),
            ("void lptd::k_path<false, true, false, false>(lptd::DScene, lptd::DProbe)", "k_path<false>"),
            ("void lptd::k_path<true, false, false, true>(lptd::DScene, lptd::DProbe)", "k_path<true>"),
            ("void lptd::k_path<0u, true>(lptd::DScene, lptd::DProbe)", "k_path<false>"),
            ("void lptd::k_path<5u, false>(lptd::DScene, lptd::DProbe)", "k_path<true>"),
            ("void lptd::k_trace<false, true, false, false>(lptd::TraceKernargs)", "k_trace<false>"),
            ("void lptd::k_trace<true, false, false, true>(lptd::TraceKernargs)", "k_trace<true>"),
            ("lptd::k_accumulate(lptd::FrameParams, HIP_vector_type<float, 4u> const*, HIP_vector_type<float, 4u>*)", "k_accumulate"),
            ("void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float> >(int)", "void at::native::vectorized_elementwise_"[:40])):
        assert short(name) == key, name


LISTING = """\t.text
\t.protected\t%(k)s ; -- Begin function %(k)s
\t.type\t%(k)s,@function
%(k)s: ; @%(k)s
; %%bb.0:
\t.loc 1 %(n)d 0
\ts_load_dword s3, s[0:1], 0xe4
\ts_cbranch_execz .LBB%(n)d_2 ; a comment
.Ltmp%(t)d:
; %%bb.1:
\tv_add_u32_e32 v4, s2, v0 ; %(k)s
\tds_read_b32 v1, v2 offset:_Z%(k)sE3lds@abs32@lo
.LBB%(n)d_2:
\ts_endpgm
\t.amdhsa_kernel %(k)s
\t\t.amdhsa_next_free_vgpr %(v)d
\t.end_amdhsa_kernel
.Lfunc_end%(n)d:
\t.size\t%(k)s, .Lfunc_end%(n)d-%(k)s
_ZN4lptd6helperEv: ; a device function: no descriptor, not a kernel
\ts_setpc_b64 s[30:31]
.Lfunc_end%(m)d:
"""


def test_kernel_bodies_sees_through_names_and_label_numbers():
    kb = _tool("kernel_bodies")
    old_name = "_ZN4lptd7k_shadeILb1ELb0ELb1ELb0ELb0ELb0ELb0EEEvNS_13ShadeKernargsE"
    new_name = "_ZN4lptd7k_shadeILj5EEEvNS_13ShadeKernargsE"
    a = kb.kernel_bodies(LISTING % dict(k=old_name, n=3, t=17, m=4, v=128))
    b = kb.kernel_bodies(LISTING % dict(k=new_name, n=40, t=2, m=41, v=128))
    c = kb.kernel_bodies(LISTING % dict(k=new_name, n=40, t=2, m=41, v=129))
    assert [n for n, _ in a] == [old_name] and [n for n, _ in b] == [new_name]          # the helper is no kernel
    assert a[0][1] == b[0][1] and len(a[0][1]) == 64
    assert c[0][1] != b[0][1]                                                            # one register more is another text
    assert kb.map_forms(old_name) == new_name and kb.map_forms(new_name) == new_name
    old_path = "_ZN4lptd6k_pathILb1ELb1ELb1ELb0EJNS_4DEnvEEEEvNS_6DSceneEiDpT3_"
    assert kb.map_forms(old_path) == "_ZN4lptd6k_pathILj3ELb1EJNS_4DEnvEEEEvNS_6DSceneEiDpT1_"
