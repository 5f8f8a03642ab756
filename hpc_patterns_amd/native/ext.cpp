// ext.cpp — pybind11 bindings for the MI355X-native core (_hpk module).
//
// Deliberately torch-free: Python passes raw device pointers
// (tensor.data_ptr()) and stream handles (torch.cuda.current_stream().
// cuda_stream, which IS a hipStream_t on ROCm), so the extension builds with
// plain hipcc, carries no torch ABI dependency, and the same library objects
// link into the standalone C++ binaries (cpp/*.cpp).

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "include/hpk.h"

namespace py = pybind11;

namespace {

hipStream_t as_stream(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

py::dict conc_bench_py(const std::string& mode,
                       const std::vector<std::string>& commands,
                       const std::map<std::string, size_t>& params,
                       bool enable_profiling, int n_queues, int n_repetitions,
                       bool verbose, int copy_engine) {
  hpk::ConcResult r;
  {
    py::gil_scoped_release release;
    r = hpk::conc_bench(mode, commands, params, enable_profiling, n_queues,
                        n_repetitions, verbose, copy_engine);
  }
  py::dict d;
  d["total_us"] = r.total_us;
  d["per_cmd_us"] = r.per_cmd_us;
  d["per_cmd_dev_ms"] = r.per_cmd_dev_ms;
  return d;
}

} // namespace

PYBIND11_MODULE(_hpk, m) {
  m.doc() = "MI355X-native HPC-patterns core (HIP/CDNA4 kernels, hipStream/"
            "hipGraph concurrency engine, xGMI topology, HIP-IPC)";

  // ---- kernels ----
  m.def("busy_wait",
        [](uintptr_t out, long tripcount, long globalsize, uintptr_t stream) {
          hpk::launch_busy_wait(reinterpret_cast<float*>(out), tripcount,
                                globalsize, as_stream(stream));
        },
        py::arg("out"), py::arg("tripcount"), py::arg("globalsize"),
        py::arg("stream") = 0);
  m.def("busy_wait_mfma",
        [](uintptr_t out, long tripcount, long n_waves, uintptr_t stream) {
          hpk::launch_busy_wait_mfma(reinterpret_cast<float*>(out), tripcount,
                                     n_waves, as_stream(stream));
        },
        py::arg("out"), py::arg("tripcount"), py::arg("n_waves"),
        py::arg("stream") = 0);
  m.def("gemm_bf16_nt",
        [](uintptr_t c, uintptr_t a, uintptr_t b, long m, long n, long k,
           uintptr_t stream, int xcd_swizzle) {
          hpk::launch_gemm_bf16_nt(reinterpret_cast<float*>(c),
                                   reinterpret_cast<const void*>(a),
                                   reinterpret_cast<const void*>(b), m, n, k,
                                   as_stream(stream), xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("m"), py::arg("n"),
        py::arg("k"), py::arg("stream") = 0, py::arg("xcd_swizzle") = 1);
  m.def("gemm_fp8_nt",
        [](uintptr_t c, uintptr_t a, uintptr_t b, long m, long n, long k,
           uintptr_t stream, int xcd_swizzle) {
          hpk::launch_gemm_fp8_nt(reinterpret_cast<float*>(c),
                                  reinterpret_cast<const void*>(a),
                                  reinterpret_cast<const void*>(b), m, n, k,
                                  as_stream(stream), xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("m"), py::arg("n"),
        py::arg("k"), py::arg("stream") = 0, py::arg("xcd_swizzle") = 0);
  m.def("gemm_i8_nt",
        [](uintptr_t c, uintptr_t a, uintptr_t b, long m, long n, long k,
           uintptr_t stream, int xcd_swizzle) {
          hpk::launch_gemm_i8_nt(reinterpret_cast<int*>(c),
                                 reinterpret_cast<const void*>(a),
                                 reinterpret_cast<const void*>(b), m, n, k,
                                 as_stream(stream), xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("m"), py::arg("n"),
        py::arg("k"), py::arg("stream") = 0, py::arg("xcd_swizzle") = 0);
  m.def("gemm_mxfp8_nt",
        [](uintptr_t c, uintptr_t a, uintptr_t b, uintptr_t as, uintptr_t bs,
           long m, long n, long k, uintptr_t stream, int xcd_swizzle) {
          hpk::launch_gemm_mxfp8_nt(reinterpret_cast<float*>(c),
                                    reinterpret_cast<const void*>(a),
                                    reinterpret_cast<const void*>(b),
                                    reinterpret_cast<const void*>(as),
                                    reinterpret_cast<const void*>(bs), m, n,
                                    k, as_stream(stream), xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("a_scale"),
        py::arg("b_scale"), py::arg("m"), py::arg("n"), py::arg("k"),
        py::arg("stream") = 0, py::arg("xcd_swizzle") = 0);
  m.def("gemm_mxfp4_nt",
        [](uintptr_t c, uintptr_t a, uintptr_t b, uintptr_t as, uintptr_t bs,
           long m, long n, long k, uintptr_t stream, int xcd_swizzle) {
          hpk::launch_gemm_mxfp4_nt(reinterpret_cast<float*>(c),
                                    reinterpret_cast<const void*>(a),
                                    reinterpret_cast<const void*>(b),
                                    reinterpret_cast<const void*>(as),
                                    reinterpret_cast<const void*>(bs), m, n,
                                    k, as_stream(stream), xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("a_scale"),
        py::arg("b_scale"), py::arg("m"), py::arg("n"), py::arg("k"),
        py::arg("stream") = 0, py::arg("xcd_swizzle") = 0);
  m.def("gemm_variant",
        [](const std::string& kind, long m, long n, long k) {
          return std::string(hpk::gemm_variant_name(kind.c_str(), m, n, k));
        },
        py::arg("kind"), py::arg("m"), py::arg("n"), py::arg("k"),
        "name of the kernel the gemm_<kind>_nt launcher runs at this shape "
        "under the current HPK_* environment");
  m.def("gemm_splitk_bf16_nt",
        [](uintptr_t c, uintptr_t a, uintptr_t b, long m, long n, long k,
           int splits, uintptr_t workspace, uintptr_t stream,
           int xcd_swizzle) {
          hpk::launch_gemm_splitk_bf16_nt(
              reinterpret_cast<float*>(c), reinterpret_cast<const void*>(a),
              reinterpret_cast<const void*>(b), m, n, k, splits,
              reinterpret_cast<void*>(workspace), as_stream(stream),
              xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("m"), py::arg("n"),
        py::arg("k"), py::arg("splits"), py::arg("workspace") = 0,
        py::arg("stream") = 0, py::arg("xcd_swizzle") = 0);
  m.def("gemm_splitk_fp8_nt",
        [](uintptr_t c, uintptr_t a, uintptr_t b, long m, long n, long k,
           int splits, uintptr_t workspace, uintptr_t stream,
           int xcd_swizzle) {
          hpk::launch_gemm_splitk_fp8_nt(
              reinterpret_cast<float*>(c), reinterpret_cast<const void*>(a),
              reinterpret_cast<const void*>(b), m, n, k, splits,
              reinterpret_cast<void*>(workspace), as_stream(stream),
              xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("m"), py::arg("n"),
        py::arg("k"), py::arg("splits"), py::arg("workspace") = 0,
        py::arg("stream") = 0, py::arg("xcd_swizzle") = 0);
  m.def("gemm_splitk_i8_nt",
        [](uintptr_t c, uintptr_t a, uintptr_t b, long m, long n, long k,
           int splits, uintptr_t workspace, uintptr_t stream,
           int xcd_swizzle) {
          hpk::launch_gemm_splitk_i8_nt(
              reinterpret_cast<int*>(c), reinterpret_cast<const void*>(a),
              reinterpret_cast<const void*>(b), m, n, k, splits,
              reinterpret_cast<void*>(workspace), as_stream(stream),
              xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("m"), py::arg("n"),
        py::arg("k"), py::arg("splits"), py::arg("workspace") = 0,
        py::arg("stream") = 0, py::arg("xcd_swizzle") = 0);
  m.def("gemm_splitk_ktiles",
        [](long t, int splits, int s) {
          if (t < 1 || splits < 1 || splits > t || s < 0 || s >= splits)
            throw py::value_error("need 1 <= splits <= T and 0 <= s < splits");
          hpk::SplitKRange r = hpk::gemm_splitk_ktiles(t, splits, s);
          return py::make_tuple(r.first, r.count);
        },
        py::arg("t"), py::arg("splits"), py::arg("s"),
        "(first, count): the K-tiles, of T = K / 64, that split s of `splits` "
        "walks; the function the kernel calls");
  m.def("gemm_splitk_plan", &hpk::gemm_splitk_plan, py::arg("m"),
        py::arg("n"), py::arg("k"), py::arg("n_cu"),
        "automatic split count for an (m, n, k) problem on n_cu compute "
        "units; pure host function");
  m.def("gemm_bf16_layout",
        [](uintptr_t c, uintptr_t a, uintptr_t b, long m, long n, long k,
           const std::string& layout, uintptr_t stream, int xcd_swizzle) {
          hpk::launch_gemm_bf16_layout(
              reinterpret_cast<float*>(c), reinterpret_cast<const void*>(a),
              reinterpret_cast<const void*>(b), m, n, k, layout.c_str(),
              as_stream(stream), xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("m"), py::arg("n"),
        py::arg("k"), py::arg("layout"), py::arg("stream") = 0,
        py::arg("xcd_swizzle") = 0,
        "layout: nn (A [M,K], B [K,N]), tn (A [K,M], B [K,N]) or tt "
        "(A [K,M], B [N,K])");
  m.def("gemm_bf16_layout_splitk",
        [](uintptr_t c, uintptr_t a, uintptr_t b, long m, long n, long k,
           const std::string& layout, int splits, uintptr_t workspace,
           uintptr_t stream, int xcd_swizzle) {
          hpk::launch_gemm_bf16_layout_splitk(
              reinterpret_cast<float*>(c), reinterpret_cast<const void*>(a),
              reinterpret_cast<const void*>(b), m, n, k, layout.c_str(),
              splits, reinterpret_cast<void*>(workspace), as_stream(stream),
              xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("m"), py::arg("n"),
        py::arg("k"), py::arg("layout"), py::arg("splits"),
        py::arg("workspace") = 0, py::arg("stream") = 0,
        py::arg("xcd_swizzle") = 0,
        "split-K over the nn / tn / tt layouts of gemm_bf16_layout; "
        "workspace [splits][M][N] fp32 when splits > 1");
  m.def("gemm_bf16_epilogue",
        [](uintptr_t c, uintptr_t a, uintptr_t b, uintptr_t bias, long m,
           long n, long k, const std::string& layout, int splits,
           uintptr_t workspace, uintptr_t stream, int xcd_swizzle) {
          hpk::launch_gemm_bf16_epilogue(
              reinterpret_cast<void*>(c), reinterpret_cast<const void*>(a),
              reinterpret_cast<const void*>(b),
              reinterpret_cast<const float*>(bias), m, n, k, layout.c_str(),
              splits, reinterpret_cast<void*>(workspace), as_stream(stream),
              xcd_swizzle);
        },
        py::arg("c"), py::arg("a"), py::arg("b"), py::arg("bias"),
        py::arg("m"), py::arg("n"), py::arg("k"), py::arg("layout"),
        py::arg("splits") = 1, py::arg("workspace") = 0,
        py::arg("stream") = 0, py::arg("xcd_swizzle") = 0,
        "C bf16 = bf16(op(A) @ op(B) + bias[n]); layout nt | nn | tn | tt, "
        "bias 0 = none; workspace [splits][M][N] fp32 when splits > 1");
  m.def("gemm_bf16_batched",
        [](uintptr_t c, int c_is_bf16, uintptr_t a, uintptr_t b, long m,
           long n, long k, long batch, long lda, long bsa, long ldb, long bsb,
           long ldc, long bsc, const std::string& layout, float alpha,
           uintptr_t stream, int xcd_swizzle) {
          hpk::launch_gemm_bf16_batched(
              reinterpret_cast<void*>(c), c_is_bf16,
              reinterpret_cast<const void*>(a),
              reinterpret_cast<const void*>(b), m, n, k, batch, lda, bsa, ldb,
              bsb, ldc, bsc, layout.c_str(), alpha, as_stream(stream),
              xcd_swizzle);
        },
        py::arg("c"), py::arg("c_is_bf16"), py::arg("a"), py::arg("b"),
        py::arg("m"), py::arg("n"), py::arg("k"), py::arg("batch"),
        py::arg("lda"), py::arg("bsa"), py::arg("ldb"), py::arg("bsb"),
        py::arg("ldc"), py::arg("bsc"), py::arg("layout"),
        py::arg("alpha") = 1.0f, py::arg("stream") = 0,
        py::arg("xcd_swizzle") = 0,
        "C_b = alpha * op(A_b) @ op(B_b), b < batch; layout nt | nn | tn | "
        "tt; ld = row stride, bs = batch stride, in elements");
  m.def("gemm_batched_c_disjoint", &hpk::gemm_batched_c_disjoint,
        py::arg("batch"), py::arg("m"), py::arg("n"), py::arg("ldc"),
        py::arg("bsc"),
        "ldc >= n and the batches' C images pairwise disjoint (batch-major "
        "or interleaved inside a row); the function the launcher calls");
  m.attr("GEMM_BATCHED_MAX_BATCH") = hpk::kGemmBatchedMaxBatch;
  m.def("gemm_bf16_act",
        [](uintptr_t c, uintptr_t aux, uintptr_t a, uintptr_t b,
           uintptr_t bias, long m, long n, long k, const std::string& layout,
           int act, int mode, int splits, uintptr_t workspace,
           uintptr_t stream, int xcd_swizzle) {
          hpk::launch_gemm_bf16_act(
              reinterpret_cast<void*>(c), reinterpret_cast<void*>(aux),
              reinterpret_cast<const void*>(a),
              reinterpret_cast<const void*>(b),
              reinterpret_cast<const float*>(bias), m, n, k, layout.c_str(),
              act, mode, splits, reinterpret_cast<void*>(workspace),
              as_stream(stream), xcd_swizzle);
        },
        py::arg("c"), py::arg("aux"), py::arg("a"), py::arg("b"),
        py::arg("bias"), py::arg("m"), py::arg("n"), py::arg("k"),
        py::arg("layout"), py::arg("act"), py::arg("mode"),
        py::arg("splits") = 1, py::arg("workspace") = 0,
        py::arg("stream") = 0, py::arg("xcd_swizzle") = 0,
        "mode ACT_FORWARD: C bf16 = bf16(act(op(A) @ op(B) + bias[n])), aux "
        "(0 = none) receives the bf16 pre-activation; mode ACT_GRAD: C = "
        "bf16((op(A) @ op(B)) * act'(aux)); act ACT_RELU | ACT_GELU (tanh)");
  m.attr("ACT_RELU") = (int)hpk::kActRelu;
  m.attr("ACT_GELU") = (int)hpk::kActGelu;
  m.attr("ACT_FORWARD") = (int)hpk::kActForward;
  m.attr("ACT_GRAD") = (int)hpk::kActGrad;
  m.def("gemm_out_lds_offset", &hpk::gemm_out_lds_offset, py::arg("row"),
        py::arg("col"),
        "byte offset of tile element (row, col) in the staged bf16 output "
        "tile; the function the kernels call");
  m.def("gemm_out_read",
        [](int t, int p, int i) {
          hpk::GemmOutRead r = hpk::gemm_out_read(t, p, i);
          return py::make_tuple(r.row, r.col);
        },
        py::arg("t"), py::arg("p"), py::arg("i"),
        "(row, col) of the first element of 16-byte LDS read i of thread t "
        "in pass p of the bf16 store loop; the function the kernels call");
  m.def("colsum_bf16",
        [](uintptr_t out, uintptr_t x, long m, long n, int chunks,
           uintptr_t workspace, uintptr_t stream) {
          hpk::launch_colsum_bf16(reinterpret_cast<float*>(out),
                                  reinterpret_cast<const void*>(x), m, n,
                                  chunks, reinterpret_cast<void*>(workspace),
                                  as_stream(stream));
        },
        py::arg("out"), py::arg("x"), py::arg("m"), py::arg("n"),
        py::arg("chunks") = 1, py::arg("workspace") = 0,
        py::arg("stream") = 0,
        "out[n] = sum_m x[m,n], x bf16 [m,n]; chunks > 1 needs a workspace "
        "of chunks * colsum_pitch(n) floats and colsum_pitch(n) floats in out");
  m.def("colsum_rows",
        [](long m, int chunks, int r) {
          if (m < 1 || chunks < 1 || chunks > m || r < 0 || r >= chunks)
            throw py::value_error("need 1 <= chunks <= M and 0 <= r < chunks");
          hpk::SplitKRange s = hpk::colsum_rows(m, chunks, r);
          return py::make_tuple(s.first, s.count);
        },
        py::arg("m"), py::arg("chunks"), py::arg("r"),
        "(first, count): the rows chunk r of `chunks` sums; the function the "
        "kernel calls");
  m.def("colsum_pitch", &hpk::colsum_pitch, py::arg("n"));
  m.def("colsum_plan", &hpk::colsum_plan, py::arg("m"), py::arg("n"),
        py::arg("n_cu"),
        "row chunks colsum_bf16 uses for an [m, n] input on n_cu compute "
        "units; pure host function");
  m.attr("COLSUM_MIN_ROWS") = hpk::kColsumMinRows;
  m.attr("COLSUM_MAX_CHUNKS") = hpk::kColsumMaxChunks;
  m.attr("SPLITK_MIN_TILES") = hpk::kSplitKMinTiles;
  m.attr("SPLITK_MAX_SPLITS") = hpk::kSplitKMaxSplits;
  m.attr("SPLITK_REDUCE_MAX_GRID") = hpk::kSplitKReduceMaxGrid;
  m.attr("QUANT_MAX_GRID") = hpk::kQuantMaxGrid;
  m.def("quantize_mx",
        [](uintptr_t q, uintptr_t scale, uintptr_t x, int x_is_bf16, int fmt,
           long rows, long k, uintptr_t stream) {
          hpk::launch_quantize_mx(reinterpret_cast<void*>(q),
                                  reinterpret_cast<void*>(scale),
                                  reinterpret_cast<const void*>(x), x_is_bf16,
                                  fmt, rows, k, as_stream(stream));
        },
        py::arg("q"), py::arg("scale"), py::arg("x"), py::arg("x_is_bf16"),
        py::arg("fmt"), py::arg("rows"), py::arg("k"), py::arg("stream") = 0,
        "fmt: 0 = mxfp8 (e4m3 bytes), 1 = mxfp4 (packed e2m1 nibbles)");
  m.def("copy_kernel",
        [](uintptr_t dst, uintptr_t src, size_t nbytes, uintptr_t stream) {
          hpk::launch_copy_kernel(reinterpret_cast<void*>(dst),
                                  reinterpret_cast<const void*>(src), nbytes,
                                  as_stream(stream));
        },
        py::arg("dst"), py::arg("src"), py::arg("nbytes"), py::arg("stream") = 0);
  m.def("copy_kernel_tuned",
        [](uintptr_t dst, uintptr_t src, size_t nbytes, uintptr_t stream,
           int unroll, size_t grid_cap) {
          hpk::launch_copy_kernel_tuned(reinterpret_cast<void*>(dst),
                                        reinterpret_cast<const void*>(src),
                                        nbytes, as_stream(stream), unroll,
                                        grid_cap);
        },
        py::arg("dst"), py::arg("src"), py::arg("nbytes"), py::arg("stream") = 0,
        py::arg("unroll") = 1, py::arg("grid_cap") = 16384);
  m.def("fill_f32",
        [](uintptr_t dst, float value, size_t n, uintptr_t stream) {
          hpk::launch_fill_f32(reinterpret_cast<float*>(dst), value, n,
                               as_stream(stream));
        },
        py::arg("dst"), py::arg("value"), py::arg("n"), py::arg("stream") = 0);
  m.def("iota_f32",
        [](uintptr_t dst, size_t n, uintptr_t stream) {
          hpk::launch_iota_f32(reinterpret_cast<float*>(dst), n,
                               as_stream(stream));
        },
        py::arg("dst"), py::arg("n"), py::arg("stream") = 0);
  m.def("acc_f32",
        [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t stream) {
          hpk::launch_acc_f32(reinterpret_cast<float*>(dst),
                              reinterpret_cast<const float*>(src), n,
                              as_stream(stream));
        },
        py::arg("dst"), py::arg("src"), py::arg("n"), py::arg("stream") = 0);
  m.def("acc_f32_nt",
        [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t stream) {
          hpk::launch_acc_f32_nt(reinterpret_cast<float*>(dst),
                                 reinterpret_cast<const float*>(src), n,
                                 as_stream(stream));
        },
        py::arg("dst"), py::arg("src"), py::arg("n"), py::arg("stream") = 0);
  m.def("reduce_sum_f32",
        [](uintptr_t src, size_t n, uintptr_t stream) {
          py::gil_scoped_release release;
          return hpk::reduce_sum_f32(reinterpret_cast<const float*>(src), n,
                                     as_stream(stream));
        },
        py::arg("src"), py::arg("n"), py::arg("stream") = 0);
  m.def("fill_i32",
        [](uintptr_t dst, int value, size_t n, uintptr_t stream) {
          hpk::launch_fill_i32(reinterpret_cast<int*>(dst), value, n,
                               as_stream(stream));
        },
        py::arg("dst"), py::arg("value"), py::arg("n"), py::arg("stream") = 0);
  m.def("acc_i32",
        [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t stream) {
          hpk::launch_acc_i32(reinterpret_cast<int*>(dst),
                              reinterpret_cast<const int*>(src), n,
                              as_stream(stream));
        },
        py::arg("dst"), py::arg("src"), py::arg("n"), py::arg("stream") = 0);
  m.def("reduce_sum_i32",
        [](uintptr_t src, size_t n, uintptr_t stream) {
          py::gil_scoped_release release;
          return hpk::reduce_sum_i32(reinterpret_cast<const int*>(src), n,
                                     as_stream(stream));
        },
        py::arg("src"), py::arg("n"), py::arg("stream") = 0);

  // ---- concurrency engine ----
  m.attr("ALLOWED_MODES") = hpk::allowed_modes;
  m.def("mode_is_allowed", &hpk::mode_is_allowed);
  m.def("conc_bench", &conc_bench_py, py::arg("mode"), py::arg("commands"),
        py::arg("params"), py::arg("enable_profiling") = false,
        py::arg("n_queues") = -1, py::arg("n_repetitions") = 10,
        py::arg("verbose") = false, py::arg("copy_engine") = 0);

  // ---- topology ----
  m.def("device_count", [] {
    py::gil_scoped_release release;
    return hpk::device_count();
  });
  m.def("link_matrix", [] {
    std::vector<std::vector<hpk::LinkInfo>> mtx;
    {
      py::gil_scoped_release release;
      mtx = hpk::link_matrix();
    }
    py::list rows;
    for (auto& row : mtx) {
      py::list r;
      for (auto& li : row) {
        py::dict d;
        d["p2p"] = li.p2p_accessible;
        d["link_type"] = li.link_type;
        d["hops"] = li.hops;
        d["min_bw_mbps"] = li.min_bw_mbps;
        d["max_bw_mbps"] = li.max_bw_mbps;
        d["weight"] = li.weight;
        r.append(d);
      }
      rows.append(r);
    }
    return rows;
  });
  m.def("p2p_planes", [] {
    py::gil_scoped_release release;
    return hpk::p2p_planes();
  });
  m.def("partition_info", [] {
    std::vector<hpk::PartitionInfo> v;
    {
      py::gil_scoped_release release;
      v = hpk::partition_info();
    }
    py::list out;
    for (auto& pi : v) {
      py::dict d;
      d["compute"] = pi.compute;
      d["memory"] = pi.memory;
      out.append(d);
    }
    return out;
  });

  // ---- IPC / peer transport ----
  m.def("ipc_get_handle", [](uintptr_t dptr) {
    auto v = hpk::ipc_get_handle(reinterpret_cast<void*>(dptr));
    return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
  });
  m.def("ipc_open_handle", [](py::bytes handle) {
    std::string s = handle;
    std::vector<uint8_t> v(s.begin(), s.end());
    return reinterpret_cast<uintptr_t>(hpk::ipc_open_handle(v));
  });
  m.def("ipc_close_handle", [](uintptr_t dptr) {
    hpk::ipc_close_handle(reinterpret_cast<void*>(dptr));
  });
  m.def("enable_peer_access", &hpk::enable_peer_access);
  m.def("sdma_num_engines", &hpk::sdma_num_engines);
  m.def("sdma_num_engines_pair", &hpk::sdma_num_engines_pair);
  m.def("sdma_copy_begin",
        [](uintptr_t dst, uintptr_t src, size_t nbytes, int device,
           int engine_index) {
          return reinterpret_cast<uintptr_t>(hpk::sdma_copy_begin(
              reinterpret_cast<void*>(dst), reinterpret_cast<const void*>(src),
              nbytes, device, engine_index));
        },
        py::arg("dst"), py::arg("src"), py::arg("nbytes"), py::arg("device") = 0,
        py::arg("engine_index") = -1);
  m.def("staged_copy",
        [](uintptr_t dst, uintptr_t src, size_t nbytes, int device,
           int engine_index, bool h2d) {
          py::gil_scoped_release release;
          hpk::staged_copy(reinterpret_cast<void*>(dst),
                           reinterpret_cast<const void*>(src), nbytes, device,
                           engine_index, h2d);
        },
        py::arg("dst"), py::arg("src"), py::arg("nbytes"), py::arg("device") = 0,
        py::arg("engine_index") = 0, py::arg("h2d") = true);
  m.def("sdma_wait", [](uintptr_t handle) {
    py::gil_scoped_release release;
    hpk::sdma_wait(reinterpret_cast<void*>(handle));
  });

  // ---- step plan: the flagship step's local commands, one submit/join ----
  py::class_<hpk::StepPlan>(m, "StepPlan")
      .def(py::init([](int device, std::tuple<uintptr_t, uintptr_t, size_t> h2d,
                       std::tuple<uintptr_t, uintptr_t, size_t> d2h,
                       std::tuple<uintptr_t, uintptr_t, size_t> d2d,
                       uintptr_t busy_out, long busy_globalsize,
                       uintptr_t busy_stream, uintptr_t copy_stream,
                       bool time_copies, double push_fraction) {
             auto triple = [](const std::tuple<uintptr_t, uintptr_t, size_t>& t) {
               return hpk::StepCopy{reinterpret_cast<void*>(std::get<0>(t)),
                                    reinterpret_cast<const void*>(std::get<1>(t)),
                                    std::get<2>(t)};
             };
             return new hpk::StepPlan(device, triple(h2d), triple(d2h),
                                      triple(d2d),
                                      reinterpret_cast<float*>(busy_out),
                                      busy_globalsize, as_stream(busy_stream),
                                      as_stream(copy_stream), time_copies,
                                      push_fraction);
           }),
           py::arg("device"), py::arg("h2d"), py::arg("d2h"), py::arg("d2d"),
           py::arg("busy_out"), py::arg("busy_globalsize"),
           py::arg("busy_stream"), py::arg("copy_stream"),
           py::arg("time_copies") = false, py::arg("push_fraction") = -1.0,
           "h2d/d2h/d2d are (dst, src, nbytes) triples of raw pointers; "
           "push_fraction < 0 leaves the host-push share of H2D to "
           "HPK_STEP_PUSH or the plan's own calibration")
      .def("submit", &hpk::StepPlan::submit, py::arg("tripcount"),
           py::call_guard<py::gil_scoped_release>())
      .def("join", &hpk::StepPlan::join,
           py::call_guard<py::gil_scoped_release>())
      .def("close", &hpk::StepPlan::close,
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("pending", &hpk::StepPlan::pending)
      .def("copy_times",
           [](const hpk::StepPlan& p) { return p.copy_times(); },
           "[(start_ns, end_ns), ...] per engine copy, H2D then D2H per "
           "submission; empty unless time_copies")
      .def("clear_copy_times", &hpk::StepPlan::clear_copy_times)
      .def_property_readonly("push_fraction", &hpk::StepPlan::push_fraction)
      .def_property_readonly("push_threads", &hpk::StepPlan::push_threads)
      .def_property_readonly("push_access", &hpk::StepPlan::push_access)
      .def("push_times", &hpk::StepPlan::push_times,
           "(wake_ns, done_ns) of the last joined step's workers, from "
           "submit entry; zeros unless time_copies")
      .def("push_probe", &hpk::StepPlan::push_probe, py::arg("reps") = 5,
           py::call_guard<py::gil_scoped_release>(),
           "[(name, value), ...]: BAR access, push rates, D2H under push "
           "(scripts/step_push_probe.py)");
  m.def("step_push_ranges",
        [](size_t nbytes, double g, int nthreads) {
          hpk::StepPushSplit s = hpk::step_push_ranges(nbytes, g, nthreads);
          return py::make_tuple(s.head, s.ranges);
        },
        py::arg("nbytes"), py::arg("g"), py::arg("nthreads"),
        "(head, [(begin, end), ...]): the engine's share of an H2D copy and "
        "the push workers' ranges; pure host function");
  m.def("hsa_timestamp_ns", &hpk::hsa_timestamp_ns);
  m.def("trace_push", [](const std::string& n) { hpk::trace_push(n.c_str()); });
  m.def("trace_pop", &hpk::trace_pop);
  m.def("trace_mark", [](const std::string& n) { hpk::trace_mark(n.c_str()); });
  m.def("memcpy_peer_async",
        [](uintptr_t dst, int dst_dev, uintptr_t src, int src_dev,
           size_t nbytes, uintptr_t stream) {
          hpk::memcpy_peer_async(reinterpret_cast<void*>(dst), dst_dev,
                                 reinterpret_cast<const void*>(src), src_dev,
                                 nbytes, as_stream(stream));
        },
        py::arg("dst"), py::arg("dst_dev"), py::arg("src"), py::arg("src_dev"),
        py::arg("nbytes"), py::arg("stream") = 0);

  // ---- raw allocation helpers (for torch-free miniapp paths/tests) ----
  m.def("hip_malloc", [](size_t nbytes) {
    void* p = nullptr;
    hpk::check_hip(hipMalloc(&p, nbytes), "hipMalloc");
    return reinterpret_cast<uintptr_t>(p);
  });
  m.def("hip_free", [](uintptr_t p) {
    hpk::check_hip(hipFree(reinterpret_cast<void*>(p)), "hipFree");
  });
  m.def("host_malloc", [](size_t nbytes) {
    void* p = nullptr;
    hpk::check_hip(hipHostMalloc(&p, nbytes, hipHostMallocDefault),
                   "hipHostMalloc");
    return reinterpret_cast<uintptr_t>(p);
  });
  m.def("host_free", [](uintptr_t p) {
    hpk::check_hip(hipHostFree(reinterpret_cast<void*>(p)), "hipHostFree");
  });
  m.def("memcpy_async",
        [](uintptr_t dst, uintptr_t src, size_t nbytes, uintptr_t stream) {
          hpk::check_hip(hipMemcpyAsync(reinterpret_cast<void*>(dst),
                                        reinterpret_cast<const void*>(src),
                                        nbytes, hipMemcpyDefault,
                                        as_stream(stream)),
                         "hipMemcpyAsync");
        });
  // kind: 1=H2D 2=D2H 3=D2D 4=default (hipMemcpyKind values) — engine
  // selection differs between Default and explicit kinds on ROCm 7.2.
  m.def("memcpy_async_kind",
        [](uintptr_t dst, uintptr_t src, size_t nbytes, int kind,
           uintptr_t stream) {
          hpk::check_hip(hipMemcpyAsync(reinterpret_cast<void*>(dst),
                                        reinterpret_cast<const void*>(src),
                                        nbytes, (hipMemcpyKind)kind,
                                        as_stream(stream)),
                         "hipMemcpyAsync(kind)");
        });
  m.def("device_synchronize", [] {
    py::gil_scoped_release release;
    hpk::check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize");
  });
  m.def("stream_synchronize", [](uintptr_t stream) {
    py::gil_scoped_release release;
    hpk::check_hip(hipStreamSynchronize(as_stream(stream)),
                   "hipStreamSynchronize");
  });
  m.def("set_device", [](int dev) {
    hpk::check_hip(hipSetDevice(dev), "hipSetDevice");
  });
}
