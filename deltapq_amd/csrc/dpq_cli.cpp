// dpq_cli.cpp -- `deltapq`, the reference-compatible command line driver for the
// query path, on top of the C-ABI (include/deltapq_amd.h).
//
// Mirrors the flag surface and output of the reference driver
// (/root/reference/deltapq_approx_tree_main.cpp:14-70 flags, :265-349 `-task
// query`, :617-710 `-task query_im`, :72-149 `-task approx_tree` with -method 1):
//
//   deltapq -dataset DIR -task query -m 8 -k 256 -h 1 -diff 8 -N 1000000
//           -query_size 1000 -topk 100 [-ext fvecs|bvecs] [-debug]
//           [-gpus G] [-out FILE]
//
// Files read from DIR, same names as the reference: M{m}K{k}codewords.txt
// (main:274), query.{ext} (main:303), M{m}K{k}_Approx_compressed_codes_opt_N{N}
// (h:2812-2814).  -h, -diff and -method are parsed and ignored by the query, as
// in the reference.  Both `query` and `query_im` load the
// index once into HBM (the reference re-opens the file per query for `query`).
// Extensions: -gpus G shards the index over G GPUs of this node and merges the
// partial top-k lists on the host; -out writes all results (the reference
// only prints top-1 under -debug); -task pqscan is the reference's uncompressed
// comparator (main:496-556); -task encode is the encode step of the reference's
// other binary, pqtree (main.cpp:314-425), so that base vectors -> codes ->
// index -> query runs from this one tool; -task learn is its learn step
// (main.cpp:243-277) with this build's own k-means (dpq_train_codebook); -task groundtruth and -task recall are
// its brute-force ground truth (main.cpp:569-669) and recall measure (main.cpp:727-803) over raw vectors, the
// latter with an optional exact re-rank of the PQ answer (-rerank R); -task decompress (no counterpart in the
// reference) decodes the DTC index on the GPU back into the codes.bin.plain record layout.  -metric l2|ip (default l2)
// switches groundtruth and recall to the inner product: dpq_flat_search_ip and its kin for the truth and the re-rank,
// dpq_query_batch_ip for the PQ answer; the truth file is then groundtruth/N{N}Top{k}.ip.txt.  -store f16|bf16 runs
// recall's re-rank a second time from the base narrowed to that format (dpq_flat_open_narrowed), -store sq8|sq4 from the
// base scalar-quantised under the quantiser trained on it (dpq_flat_open_quantised).
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/deltapq_amd.h"

static double Elapsed() {  // utils.cpp:112-116
    using namespace std::chrono;
    return duration<double>(system_clock::now().time_since_epoch()).count();
}

static int die(const char* where, int rc) {
    std::cout << where << ": " << dpq_strerror(rc) << ": " << dpq_last_error() << std::endl;
    return 1;
}

// -filter FILE: a bitmap over original vector ids (dpq_write_bitmap's format).
static int read_filter(const std::string& path, std::vector<uint32_t>* words, int64_t* n_bits) {
    int rc = dpq_read_bitmap(path.c_str(), n_bits, nullptr);
    if (rc) return rc;
    words->assign((size_t)((*n_bits + 31) / 32) + 1, 0u);
    return dpq_read_bitmap(path.c_str(), n_bits, words->data());
}

// -opq: the rows are replaced by rows . R on GPU 0 (dpq_rotate), R from M{M}K{K}rotation.fvecs beside the codewords.
// A missing or unreadable file is an error that names the file.
static int rotate_rows(const std::string& dataset, int M, int K, std::vector<float>* rows, int64_t n, int D) {
    const std::string path = dataset + "/M" + std::to_string(M) + "K" + std::to_string(K) + "rotation.fvecs";
    int32_t rD = 0;
    int rc = dpq_read_rotation(path.c_str(), &rD, nullptr);
    if (rc) {
        std::cout << "-opq: cannot read the rotation file " << path << " (written by -task learn -opq T): " << dpq_strerror(rc)
                  << ": " << dpq_last_error() << std::endl;
        return 1;
    }
    if (rD != D) {
        std::cout << "-opq: " << path << " is " << rD << " x " << rD << " but the vectors have " << D << " dimensions" << std::endl;
        return 1;
    }
    std::vector<float> R((size_t)D * D), out((size_t)n * D);
    rc = dpq_read_rotation(path.c_str(), &rD, R.data());
    if (rc) return die("dpq_read_rotation", rc);
    rc = dpq_rotate(rows->data(), n, D, R.data(), 0, out.data());
    if (rc) return die("dpq_rotate", rc);
    rows->swap(out);
    return 0;
}

int main(int argc, char* argv[]) {
    std::string dataset, queryset, task = "approx_tree", ext = "fvecs", out_path, order = "dfs", filter_path, init = "rows";
    std::string metric = "l2", store;
    int query_size = -1, top_k = 1, diff_argument = 1, debug = 0, max_height_folds = 1, method = 1;
    int PQ_M = 0, PQ_K = 0, gpus = 1, gt_topk = -1, rerank = 0;
    bool topk_given = false;
    long long N = -1;
    int restarts = 1;
    unsigned long long seed = 0;
    int refine_m2 = 0, refine_k2 = 0, refine_r = 0;
    long long train_size = 0;
    bool opq = false;
    int opq_outer = 0, opq_init_iters = 25, opq_inner_iters = 4;
    std::string ivf_path;
    int nprobe = 1, learn_nlist = 0, iters = 25;
    for (int i = 0; i < argc; i++) {  // main:26-70: hand-rolled scan, no validation
        std::string arg = argv[i];
        const char* nx = i + 1 < argc ? argv[i + 1] : "";
        if (arg == "-dataset") dataset = nx;
        if (arg == "-queryset") queryset = nx;
        if (arg == "-task") task = nx;
        if (arg == "-topk") top_k = atoi(nx), topk_given = true;
        if (arg == "-gt_topk") gt_topk = atoi(nx);
        if (arg == "-rerank") rerank = atoi(nx);
        if (arg == "-filter") filter_path = nx;
        if (arg == "-metric") metric = nx;
        if (arg == "-store") store = nx;
        if (arg == "-N") N = atoll(nx);
        if (arg == "-diff") diff_argument = atoi(nx);
        if (arg == "-query_size") query_size = atoi(nx);
        if (arg == "-m") PQ_M = atoi(nx);
        if (arg == "-k") PQ_K = atoi(nx);
        if (arg == "-ext") ext = nx;
        if (arg == "-debug") debug = 1;
        if (arg == "-h") max_height_folds = atoi(nx);  // max height folds, not help (main:61-63)
        if (arg == "-method") method = atoi(nx);
        if (arg == "-gpus") gpus = atoi(nx);
        if (arg == "-out") out_path = nx;
        if (arg == "-order") order = nx;
        if (arg == "-init") init = nx;
        if (arg == "-restarts") restarts = atoi(nx);
        if (arg == "-seed") seed = strtoull(nx, nullptr, 10);
        if (arg == "-m2") refine_m2 = atoi(nx);
        if (arg == "-k2") refine_k2 = atoi(nx);
        if (arg == "-refine") refine_r = atoi(nx);
        if (arg == "-train_size") train_size = atoll(nx);
        if (arg == "-opq") opq = true, opq_outer = atoi(nx);  // learn: -opq T outer steps; elsewhere a bare flag
        if (arg == "-opq_init_iters") opq_init_iters = atoi(nx);
        if (arg == "-opq_inner_iters") opq_inner_iters = atoi(nx);
        if (arg == "-ivf") ivf_path = nx;
        if (arg == "-nprobe") nprobe = atoi(nx);
        if (arg == "-nlist") learn_nlist = atoi(nx);
        if (arg == "-iters") iters = atoi(nx);
    }
    (void)diff_argument; (void)method; (void)queryset;
    if (opq && (task == "refine" || (task == "recall" && refine_r != 0))) {
        std::cout << "usage: -opq cannot be combined with -task refine or -refine R: a refine level over rotated codes is out of "
                     "scope" << std::endl;
        return 2;
    }

    // -metric hamming: exact Hamming distances over packed bits, eight dimensions to a byte of a .bvecs file
    const bool hamming = metric == "hamming";
    if (hamming && (task != "groundtruth" || ext != "bvecs")) {
        std::cout << "usage: -metric hamming serves -task groundtruth -ext bvecs [-filter FILE]: base.bvecs and query.bvecs hold "
                     "packed bits, every byte eight dimensions (dimension d in bit d & 7 of byte d >> 3); a .fvecs file has no bits"
                  << std::endl;
        return 2;
    }
    const bool ip = metric == "ip";
    if ((!ip && !hamming && metric != "l2") || (ip && (refine_r != 0 || gpus > 1 || (task != "groundtruth" && task != "recall")))) {
        std::cout << "usage: -metric l2|ip|hamming (default l2); -metric hamming serves -task groundtruth -ext bvecs; -metric ip serves -task groundtruth and -task recall [-rerank R] "
                     "[-filter FILE] [-opq] [-ivf FILE -nprobe P], and cannot be combined with -refine R or -gpus above 1" << std::endl;
        return 2;
    }

    const bool store_sq = store == "sq8" || store == "sq4";
    if (!store.empty() && ((store != "f16" && store != "bf16" && !store_sq) || task != "recall" || rerank == 0)) {
        std::cout << "usage: -store f16|bf16|sq8|sq4 serves -task recall with -rerank R (also with -metric ip): the re-rank is "
                     "run a second time from the base narrowed to that format (dpq_flat_open_narrowed), or scalar-quantised to 8 "
                     "or 4 bits per dimension under the quantiser trained on the base itself (dpq_flat_open_quantised), and its "
                     "recall printed beside the fp32 line" << std::endl;
        return 2;
    }

    if (task == "learn") {
        // The other binary's `pqtree -task learn` (main.cpp:243-277): learn.{ext} -> M{M}K{K}codewords.txt.  The
        // reference shuffles the file's vectors before it takes -N of them (main.cpp:262) and trains with cv::kmeans;
        // here -N takes the first N vectors as they are and dpq_train_codebook trains with its own stated rules.
        // -init rows|pp: K random rows or k-means++; -restarts R: the best of R runs per sub-space; -seed S.
        if (PQ_M <= 0 || PQ_K <= 0 || dataset.empty() || (init != "rows" && init != "pp")) {
            std::cout << "usage: deltapq -dataset DIR -task learn -m M -k K [-N TRAIN_SIZE] [-ext fvecs|bvecs] [-init rows|pp] "
                         "[-restarts R] [-seed S] [-opq T [-opq_init_iters A] [-opq_inner_iters B]]" << std::endl;
            return 2;
        }
        const std::string learn_path = dataset + "/learn." + ext;  // main.cpp:251
        int64_t n_file = 0;
        int32_t D = 0;
        int rc = dpq_read_vecs(learn_path.c_str(), ext == "bvecs", &n_file, &D, nullptr, 0);
        if (rc) return die("ReadTopN", rc);
        int64_t n = n_file;
        if (N != -1 && N < n) n = N;
        std::vector<float> learn((size_t)n * D);
        rc = dpq_read_vecs(learn_path.c_str(), ext == "bvecs", &n_file, &D, learn.data(), n);
        if (rc) return die("ReadTopN", rc);
        const int Ds = (D + PQ_M - 1) / PQ_M;
        std::vector<float> codewords((size_t)PQ_M * PQ_K * Ds);
        const std::string cw_path =
            dataset + "/M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) + "codewords.txt";  // main.cpp:273-275
        if (opq) {
            // -opq T: OPQ (dpq_opq_train): T outer steps around the trainer; the codebook is that of the rotated space and
            // the rotation goes to M{M}K{K}rotation.fvecs beside it
            std::vector<float> rotation((size_t)D * D);
            dpq_opq_opts oo = {};
            oo.outer_iters = opq_outer;
            oo.init_iters = opq_init_iters;
            oo.inner_iters = opq_inner_iters;
            oo.seed = seed;
            oo.init = init == "pp" ? 1 : 0;
            oo.restarts = restarts;
            dpq_opq_stats os;
            rc = dpq_opq_train(learn.data(), n, D, PQ_M, PQ_K, &oo, rotation.data(), codewords.data(), &os);
            if (rc) return die("learn -opq", rc);
            for (int t = 0; t <= os.outer_run; ++t) std::cout << "outer step " << t << " objective " << os.objective[t] << std::endl;
            const std::string rot_path =
                dataset + "/M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) + "rotation.fvecs";
            rc = dpq_write_codewords(cw_path.c_str(), codewords.data(), PQ_M, PQ_K, Ds);
            if (rc) return die("PQ::WriteCodewords", rc);
            rc = dpq_write_rotation(rot_path.c_str(), rotation.data(), D);
            if (rc) return die("dpq_write_rotation", rc);
            std::cout << "learned OPQ M = " << PQ_M << " K = " << PQ_K << " Ds = " << Ds << " from " << n << " vectors: step "
                      << os.best_t << " of " << os.outer_run << " kept, " << os.degenerate << " degenerate, " << os.wall_ms / 1000
                      << " [sec] -> " << cw_path << ", " << rot_path << std::endl;
            return 0;
        }
        dpq_train_stats st;
        dpq_train_opts topts = {};
        topts.max_iters = 25;
        topts.seed = seed;
        topts.init = init == "pp" ? 1 : 0;
        topts.restarts = restarts;
        rc = dpq_train_codebook(learn.data(), n, D, PQ_M, PQ_K, &topts, codewords.data(), &st);
        if (rc) return die("learn", rc);
        for (int r = 0; r < st.iters_run; ++r) std::cout << "round " << r + 1 << " distortion " << st.distortion[r] << std::endl;
        rc = dpq_write_codewords(cw_path.c_str(), codewords.data(), PQ_M, PQ_K, Ds);
        if (rc) return die("PQ::WriteCodewords", rc);
        std::cout << "learned M = " << PQ_M << " K = " << PQ_K << " Ds = " << Ds << " from " << n << " vectors in " << st.iters_run
                  << " rounds" << (st.converged ? " (converged)" : "") << ", " << st.reseeded << " empty clusters reseeded, "
                  << st.wall_ms / 1000 << " [sec] -> " << cw_path << std::endl;
        return 0;
    }
    if (task == "ivf_learn") {
        // No reference counterpart: learn.fvecs -> IVF{L}centroids.fvecs, the coarse quantiser `-task recall -ivf FILE` takes
        // (dpq_ivf_train: Lloyd's rounds over whole vectors, the seeded-rows start).  -N takes the first T vectors.
        if (learn_nlist <= 0 || dataset.empty()) {
            std::cout << "usage: deltapq -dataset DIR -task ivf_learn -nlist L [-N TRAIN_SIZE] [-iters I] [-seed S]" << std::endl;
            return 2;
        }
        const std::string learn_path = dataset + "/learn.fvecs";
        int64_t n_file = 0;
        int32_t D = 0;
        int rc = dpq_read_vecs(learn_path.c_str(), 0, &n_file, &D, nullptr, 0);
        if (rc) return die("ReadTopN", rc);
        int64_t n = n_file;
        if (N != -1 && N < n) n = N;
        std::vector<float> learn((size_t)n * D);
        rc = dpq_read_vecs(learn_path.c_str(), 0, &n_file, &D, learn.data(), n);
        if (rc) return die("ReadTopN", rc);
        std::vector<float> centroids((size_t)learn_nlist * D);
        dpq_ivf_train_opts io = {};
        io.max_iters = iters;
        io.seed = seed;
        dpq_ivf_train_stats st;
        rc = dpq_ivf_train(learn.data(), n, D, learn_nlist, &io, centroids.data(), &st);
        if (rc) return die("ivf_learn", rc);
        for (int r = 0; r < st.iters_run; ++r) std::cout << "round " << r + 1 << " distortion " << st.distortion[r] << std::endl;
        const std::string out = dataset + "/IVF" + std::to_string(learn_nlist) + "centroids.fvecs";
        rc = dpq_write_vecs(out.c_str(), centroids.data(), learn_nlist, D);
        if (rc) return die("dpq_write_vecs", rc);
        std::cout << "assign " << st.assign_ms << " [ms] update " << st.update_ms << " [ms] repair " << st.repair_ms
                  << " [ms] rounds " << st.rounds_ms << " [ms]" << std::endl;
        std::cout << "learned nlist = " << learn_nlist << " D = " << D << " from " << n << " vectors in " << st.iters_run << " rounds"
                  << (st.converged ? " (converged)" : "") << ", " << st.reseeded << " empty lists reseeded, " << st.wall_ms / 1000
                  << " [sec] -> " << out << std::endl;
        return 0;
    }
    if (task == "encode") {
        // The other binary's `pqtree -task encode` (main.cpp:314-425): base.{ext} -> PQ codes (nearest
        // codeword per sub-space, PQTree::EncodePlain pq_tree.cpp:215-237) -> codes.bin.plain.M{M}K{K}N{N}.
        if (PQ_M <= 0 || PQ_K <= 0 || dataset.empty()) {
            std::cout << "usage: deltapq -dataset DIR -task encode -m M -k K [-N N] [-ext fvecs|bvecs] [-opq]" << std::endl;
            return 2;
        }
        const std::string cw_path =
            dataset + "/M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) + "codewords.txt";
        int32_t cM = 0, cK = 0, cDs = 0;
        int rc = dpq_read_codewords(cw_path.c_str(), &cM, &cK, &cDs, nullptr);
        if (rc) return die("ReadCodewords", rc);
        std::vector<float> codewords((size_t)cM * cK * cDs);
        rc = dpq_read_codewords(cw_path.c_str(), &cM, &cK, &cDs, codewords.data());
        if (rc) return die("ReadCodewords", rc);
        if (cM != PQ_M || cK != PQ_K) {
            std::cout << "codewords file is M=" << cM << " K=" << cK << std::endl;
            return 1;
        }
        const std::string base_path = dataset + "/base." + ext;  // main.cpp:354
        int64_t n_file = 0;
        int32_t D = 0;
        rc = dpq_read_vecs(base_path.c_str(), ext == "bvecs", &n_file, &D, nullptr, 0);
        if (rc) return die("ItrReader", rc);
        int64_t n = n_file;
        if (N != -1 && N < n) n = N;  // main.cpp:339-340: -N caps the number of vectors
        std::vector<float> base((size_t)n * D);
        rc = dpq_read_vecs(base_path.c_str(), ext == "bvecs", &n_file, &D, base.data(), n);
        if (rc) return die("ItrReader", rc);
        if (opq && rotate_rows(dataset, PQ_M, PQ_K, &base, n, D)) return 1;  // the codes are those of the rotated vectors
        const double t0 = Elapsed();
        std::vector<uint8_t> codes((size_t)n * PQ_M);
        rc = dpq_encode_pq(base.data(), n, D, codewords.data(), PQ_M, PQ_K, cDs, 0, codes.data());
        if (rc) return die("encode", rc);
        const std::string out = dataset + "/codes.bin.plain.M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) +
                                "N" + std::to_string(n);  // main.cpp:409-411
        rc = dpq_write_codes_plain(out.c_str(), codes.data(), n, PQ_M);
        if (rc) return die("PQTree::Write", rc);
        std::cout << "N = " << n << std::endl;                                         // pq_tree.cpp:1021
        std::cout << "encoded " << n << " vectors in " << (Elapsed() - t0) << " [sec] -> " << out << std::endl;
        return 0;
    }
    if (task == "approx_tree") {
        // main:72-149: codes.bin.plain -> DeltaTree -> the three index artefacts
        if (PQ_M <= 0 || PQ_K <= 0 || dataset.empty() || N < 0) {
            std::cout << "usage: deltapq -dataset DIR -task approx_tree -m M -k K -N N [-h FOLDS]" << std::endl;
            return 2;
        }
        std::cout << "M = " << PQ_M << std::endl;
        const std::string codes_path = dataset + "/codes.bin.plain.M" + std::to_string(PQ_M) + "K" +
                                       std::to_string(PQ_K) + "N" + std::to_string(N);  // main:76-77
        int64_t NN = 0;
        int rc = dpq_read_codes_plain(codes_path.c_str(), PQ_M, &NN, nullptr);
        if (rc) return die("PQTree::Read", rc);
        std::cout << "Read: N = " << NN << std::endl;
        std::vector<uint8_t> vecs((size_t)NN * PQ_M);
        rc = dpq_read_codes_plain(codes_path.c_str(), PQ_M, &NN, vecs.data());
        if (rc) return die("PQTree::Read", rc);
        const std::string cw_path =
            dataset + "/M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) + "codewords.txt";  // main:88-89
        int32_t cM = 0, cK = 0, cDs = 0;
        rc = dpq_read_codewords(cw_path.c_str(), &cM, &cK, &cDs, nullptr);
        if (rc) return die("ReadCodewords", rc);
        std::vector<float> codewords((size_t)cM * cK * cDs);
        rc = dpq_read_codewords(cw_path.c_str(), &cM, &cK, &cDs, codewords.data());
        if (rc) return die("ReadCodewords", rc);
        if (cM != PQ_M || cK != PQ_K) {
            std::cout << "codewords file is M=" << cM << " K=" << cK << std::endl;
            return 1;
        }
        std::cout << "K = " << PQ_K << std::endl << "N = " << NN << std::endl << dataset << std::endl;
        const double t0 = Elapsed();  // main:98
        dpq_tree* tree = nullptr;
        // the sort/group passes run on GPU 0 when there is one (same tree either way); -cpu_build forces the host
        bool cpu_build = dpq_device_count() < 1;
        for (int i = 0; i < argc; i++)
            if (std::string(argv[i]) == "-cpu_build") cpu_build = true;
        std::cout << "edge search on " << (cpu_build ? "the host" : "GPU 0") << std::endl;
        rc = cpu_build ? dpq_tree_build(vecs.data(), NN, PQ_M, PQ_K, max_height_folds, codewords.data(), cDs, &tree)
                       : dpq_tree_build_gpu(vecs.data(), NN, PQ_M, PQ_K, max_height_folds, codewords.data(), cDs, 0,
                                            &tree);
        if (rc) return die("create_approx_tree", rc);
        dpq_dtc_stats st;
        dpq_tree_stats(tree, &st);
        std::cout << "   ++++ TOTAL number of Diffs " << st.n_diffs << std::endl;                       // h:1315
        for (int d = 0; d < PQ_M + 2 && d < 16; ++d) std::cout << st.depth_hist[d] << " nodes at depth " << d << std::endl;  // h:1467-1469
        std::cout << "number of bytes is " << st.n_bytes << std::endl;                                  // h:1768
        rc = dpq_tree_write_files(tree, dataset.c_str());
        if (rc) return die("write index files", rc);
        dpq_tree_free(tree);
        std::cout << "==========================BUILD DELTATREE INDEX IN " << (Elapsed() - t0) << " [sec] "
                  << "==========================" << std::endl << std::endl;                           // main:136-137
        std::cout << "WARNING: Just built an index. no query processed." << std::endl;                 // main:140
        return 0;
    }
    if (task == "decompress") {
        // No counterpart in the reference (it never reads a code back out of its index): the DTC index decoded on the
        // GPU (dpq_decode_range over everything) into the codes.bin.plain record layout, in DFS order or -- through the
        // TreeNodesDFS file's vec_ids -- in the order of the encoder's file.
        if (PQ_M <= 0 || PQ_K <= 0 || dataset.empty() || N < 0 || (order != "dfs" && order != "file")) {
            std::cout << "usage: deltapq -dataset DIR -task decompress -m M -k K -N N [-order dfs|file]" << std::endl;
            return 2;
        }
        char path[4096];
        int rc = dpq_dtc_file_name(dataset.c_str(), PQ_M, PQ_K, N, path, sizeof path);
        if (rc) return die("dpq_dtc_file_name", rc);
        const double t0 = Elapsed();
        dpq_index* idx = nullptr;
        rc = dpq_open_file(path, PQ_M, PQ_K, nullptr, &idx);
        if (rc) return die("dpq_open_file", rc);
        dpq_info inf;
        dpq_get_info(idx, &inf);
        const int64_t n = inf.node_hi - inf.node_lo;
        std::vector<uint8_t> codes((size_t)n * PQ_M);
        rc = dpq_decode_range(idx, inf.node_lo, n, codes.data());
        dpq_close(idx);
        if (rc) return die("dpq_decode_range", rc);
        if (order == "file") {
            if (PQ_M > 8) {
                std::cout << "-order file needs the TreeNodesDFS file, which exists for M <= 8 only" << std::endl;
                return 1;
            }
            const std::string nodes_path = dataset + "/M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) +
                                           "_Approx_TreeNodesDFS_N" + std::to_string(N);
            std::vector<uint32_t> vec_id((size_t)n);
            rc = dpq_read_qnode_ids(nodes_path.c_str(), n, vec_id.data());
            if (rc) return die("dpq_read_qnode_ids", rc);
            std::vector<uint8_t> by_file((size_t)n * PQ_M);
            std::vector<bool> seen((size_t)n, false);
            for (int64_t p = 0; p < n; ++p) {
                const uint32_t v = vec_id[(size_t)p];
                if (v >= (uint64_t)n || seen[v]) {
                    std::cout << nodes_path << ": vec_ids are not a permutation of 0.." << n - 1 << std::endl;
                    return 1;
                }
                seen[v] = true;
                memcpy(&by_file[(size_t)v * PQ_M], &codes[(size_t)p * PQ_M], (size_t)PQ_M);
            }
            codes.swap(by_file);
        }
        const std::string out = dataset + "/codes.bin.decoded.M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) + "N" +
                                std::to_string(N);
        rc = dpq_write_codes_plain(out.c_str(), codes.data(), n, PQ_M);
        if (rc) return die("PQTree::Write", rc);
        std::cout << "decoded " << n << " codes (" << order << " order) in " << (Elapsed() - t0) << " [sec] -> " << out
                  << std::endl;
        return 0;
    }
    if (task == "groundtruth") {
        // The other binary's `pqtree -task groundtruth` (main.cpp:569-669): brute force over base.{ext}, streamed in
        // parts; every part is a dpq_flat handle with its own id offset, the partial lists meet in dpq_merge_topk_host.
        // With -ext bvecs the bytes stay bytes (dpq_flat_open_u8 / dpq_flat_search[_ip]_u8): the same bits, the same file.
        if (dataset.empty() || !topk_given || top_k < 1 || query_size < 1) {
            std::cout << "usage: deltapq -dataset DIR -task groundtruth -topk K -query_size Q [-N N] [-ext fvecs|bvecs] [-filter FILE]"
                         " [-metric l2|ip|hamming]" << std::endl;
            return 2;
        }
        // -metric hamming: the bytes are packed bits, D = 8 x the file's dimension (dpq_flat_open_bits / dpq_flat_search_bits)
        // -metric ip: exact inner products (dpq_flat_search_ip; over a .bvecs base dpq_flat_search_ip_u8, the bytes kept)
        const bool file_bvecs = ext == "bvecs", bvecs = file_bvecs;
        const std::string q_path = dataset + "/query." + ext, base_path = dataset + "/base." + ext;
        int64_t nq_file = 0, n_file = 0;
        int32_t D = 0, Db = 0;
        int rc = DPQ_OK;
        // -filter FILE: the exact top-k among the vectors the bitmap allows, one filter per part from the same bitmap
        const bool filtered = !filter_path.empty();
        std::vector<uint32_t> f_words;
        int64_t f_bits = 0;
        if (filtered && (rc = read_filter(filter_path, &f_words, &f_bits))) return die("dpq_read_bitmap", rc);
        rc = dpq_read_vecs(q_path.c_str(), file_bvecs, &nq_file, &D, nullptr, 0);
        if (rc) return die("ReadTopN", rc);
        if (query_size > nq_file) {
            std::cout << "-query_size " << query_size << " exceeds the " << nq_file << " available queries" << std::endl;
            return 1;
        }
        const int nq = query_size;
        std::vector<float> queries;    // -ext fvecs
        std::vector<uint8_t> queries8;  // -ext bvecs: the bytes stay bytes
        if (bvecs) {
            queries8.resize((size_t)nq * D);
            rc = dpq_read_bvecs_range(q_path.c_str(), 0, nq, &D, queries8.data());
        } else {
            queries.resize((size_t)nq * D);
            rc = dpq_read_vecs(q_path.c_str(), file_bvecs, &nq_file, &D, queries.data(), nq);
        }
        if (rc) return die("ReadTopN", rc);
        rc = dpq_read_vecs(base_path.c_str(), file_bvecs, &n_file, &Db, nullptr, 0);
        if (rc) return die("ItrReader", rc);
        if (Db != D) {
            std::cout << "query dimension " << D << " != base dimension " << Db << std::endl;
            return 1;
        }
        int64_t n = n_file;
        if (N != -1 && N < n) n = N;
        if (top_k > n || top_k > DPQ_FLAT_MAX_TOPK) {
            std::cout << "-topk " << top_k << " outside 1.." << std::min<int64_t>(n, DPQ_FLAT_MAX_TOPK) << std::endl;
            return 1;
        }
        if (hamming && D > DPQ_FLAT_BITS_MAX_D / 8) {
            std::cout << "-metric hamming: " << D << " bytes a row exceed " << DPQ_FLAT_BITS_MAX_D << " bits" << std::endl;
            return 1;
        }
        if (dpq_device_count() < 1) {
            std::cout << "no GPU visible: this build has no CPU search path" << std::endl;
            return 1;
        }
        // at most 2 GB per part: of floats, or with -ext bvecs of bytes (a byte handle, four times as many rows)
        int64_t part_rows = std::max<int64_t>(1, ((int64_t)1 << (bvecs ? 31 : 29)) / D);
        std::vector<uint8_t> part8;
        if (const char* dev = getenv("DPQ_DEV"))
            if (atoi(dev) != 0)
                if (const char* e = getenv("DPQ_GT_PART_ROWS")) part_rows = std::max<int64_t>(1, atoll(e));  // developer knob
        const size_t list = (size_t)nq * top_k;
        std::vector<int32_t> two_ids(2 * list, -1), out_ids(list);  // [0] the answer so far, [1] the part's
        const float pad = ip ? -INFINITY : INFINITY;
        std::vector<float> two_dists(2 * list, pad), out_dists(list);
        std::vector<float> part;
        std::vector<int32_t> p_ids;
        std::vector<float> p_dists;
        const double t0 = Elapsed();
        int n_parts = 0;
        for (int64_t r0 = 0; r0 < n; r0 += part_rows, ++n_parts) {
            const int64_t rows = std::min(part_rows, n - r0);
            dpq_flat* f = nullptr;
            if (bvecs) {
                part8.resize((size_t)rows * D);
                rc = dpq_read_bvecs_range(base_path.c_str(), r0, rows, &Db, part8.data());
                if (rc) return die("ItrReader", rc);
                rc = hamming ? dpq_flat_open_bits(part8.data(), rows, 8 * D, 0, r0, &f) : dpq_flat_open_u8(part8.data(), rows, D, 0, r0, &f);
            } else {
                part.resize((size_t)rows * D);
                rc = dpq_read_vecs_range(base_path.c_str(), file_bvecs, r0, rows, &Db, part.data());
                if (rc) return die("ItrReader", rc);
                rc = dpq_flat_open(part.data(), rows, D, 0, r0, &f);
            }
            if (rc) return die(hamming ? "dpq_flat_open_bits" : bvecs ? "dpq_flat_open_u8" : "dpq_flat_open", rc);
            // a short last part gives a short list, padded; a filtered search pads its own rows
            const int kk = filtered ? top_k : (int)std::min<int64_t>(top_k, rows);
            p_ids.resize((size_t)nq * kk);
            p_dists.resize((size_t)nq * kk);
            if (filtered) {
                dpq_flat_filter* ff = nullptr;
                rc = dpq_flat_filter_create(f, f_words.data(), f_bits, &ff);
                if (rc) return die("dpq_flat_filter_create", rc);
                rc = hamming ? dpq_flat_search_filtered_bits(f, ff, queries8.data(), nq, kk, p_ids.data(), p_dists.data())
                     : bvecs ? (ip ? dpq_flat_search_filtered_ip_u8(f, ff, queries8.data(), nq, kk, p_ids.data(), p_dists.data())
                                 : dpq_flat_search_filtered_u8(f, ff, queries8.data(), nq, kk, p_ids.data(), p_dists.data()))
                     : ip  ? dpq_flat_search_filtered_ip(f, ff, queries.data(), nq, kk, p_ids.data(), p_dists.data())
                           : dpq_flat_search_filtered(f, ff, queries.data(), nq, kk, p_ids.data(), p_dists.data());
                if (rc)
                    return die(hamming ? "dpq_flat_search_filtered_bits"
                               : bvecs ? (ip ? "dpq_flat_search_filtered_ip_u8" : "dpq_flat_search_filtered_u8")
                               : ip  ? "dpq_flat_search_filtered_ip"
                                     : "dpq_flat_search_filtered", rc);
                dpq_flat_filter_free(ff);
            } else {
                rc = hamming ? dpq_flat_search_bits(f, queries8.data(), nq, kk, p_ids.data(), p_dists.data())
                     : bvecs ? (ip ? dpq_flat_search_ip_u8(f, queries8.data(), nq, kk, p_ids.data(), p_dists.data())
                                 : dpq_flat_search_u8(f, queries8.data(), nq, kk, p_ids.data(), p_dists.data()))
                     : ip  ? dpq_flat_search_ip(f, queries.data(), nq, kk, p_ids.data(), p_dists.data())
                           : dpq_flat_search(f, queries.data(), nq, kk, p_ids.data(), p_dists.data());
                if (rc)
                    return die(hamming ? "dpq_flat_search_bits"
                               : bvecs ? (ip ? "dpq_flat_search_ip_u8" : "dpq_flat_search_u8") : ip ? "dpq_flat_search_ip" : "dpq_flat_search",
                               rc);
            }
            dpq_flat_close(f);
            for (int q = 0; q < nq; ++q)
                for (int r = 0; r < top_k; ++r) {
                    two_ids[list + (size_t)q * top_k + r] = r < kk ? p_ids[(size_t)q * kk + r] : -1;
                    two_dists[list + (size_t)q * top_k + r] = r < kk ? p_dists[(size_t)q * kk + r] : pad;
                }
            rc = ip ? dpq_merge_topk_ip_host(two_ids.data(), two_dists.data(), 2, nq, top_k, out_ids.data(), out_dists.data())
                    : dpq_merge_topk_host(two_ids.data(), two_dists.data(), 2, nq, top_k, out_ids.data(), out_dists.data());
            if (rc) return die(ip ? "dpq_merge_topk_ip_host" : "dpq_merge_topk_host", rc);
            std::copy(out_ids.begin(), out_ids.end(), two_ids.begin());
            std::copy(out_dists.begin(), out_dists.end(), two_dists.begin());
        }
        const double elapsed = Elapsed() - t0;
        std::cout << n << " base vectors in " << n_parts << " part(s)" << std::endl;
        std::cout << elapsed / (double)nq * 1000 << " [msec/query] " << std::endl;
        const std::string gt_dir = dataset + "/groundtruth";
        mkdir(gt_dir.c_str(), 0777);  // (exists already: fine)
        const std::string gt_path = gt_dir + "/N" + std::to_string(n) + "Top" + std::to_string(top_k) +
                                    (ip ? ".ip" : hamming ? ".hamming" : "") + (filtered ? ".filtered.txt" : ".txt");  // main.cpp:663-667
        rc = dpq_write_groundtruth(gt_path.c_str(), out_ids.data(), out_dists.data(), nq, top_k);
        if (rc) return die("write_groundtruth", rc);
        std::cout << gt_path << std::endl;
        return 0;
    }
    if (task == "refine") {
        // A second PQ level over the residuals of the index's nodes (dpq_refine_build): base.{ext}, the DTC index, its
        // codewords and the TreeNodesDFS file (DFS position -> vector id, written for M <= 8 only) ->
        // M{M}K{K}_refine_M{M2}K{K2}codewords.txt and codes.bin.refine.M{M}K{K}M{M2}K{K2}N{N}.
        if (PQ_M <= 0 || PQ_K <= 0 || dataset.empty() || N < 1) {
            std::cout << "usage: deltapq -dataset DIR -task refine -m M -k K -N N [-m2 M2] [-k2 K2] [-train_size T] [-seed S]"
                         " [-ext fvecs|bvecs]   (M <= 8: the TreeNodesDFS file supplies the vector ids)" << std::endl;
            return 2;
        }
        if (PQ_M > 8) {
            std::cout << "-task refine needs M <= 8: there is no TreeNodesDFS file (vector ids) at M = " << PQ_M << std::endl;
            return 1;
        }
        const bool bvecs = ext == "bvecs";
        const std::string cw_path = dataset + "/M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) + "codewords.txt";
        int32_t cM = 0, cK = 0, cDs = 0;
        int rc = dpq_read_codewords(cw_path.c_str(), &cM, &cK, &cDs, nullptr);
        if (rc) return die("ReadCodewords", rc);
        std::vector<float> codewords((size_t)cM * cK * cDs);
        rc = dpq_read_codewords(cw_path.c_str(), &cM, &cK, &cDs, codewords.data());
        if (rc) return die("ReadCodewords", rc);
        if (cM != PQ_M || cK != PQ_K) {
            std::cout << "codewords file is M=" << cM << " K=" << cK << std::endl;
            return 1;
        }
        const std::string base_path = dataset + "/base." + ext;
        int32_t D = 0;
        rc = dpq_read_vecs_range(base_path.c_str(), bvecs, 0, N, &D, nullptr);
        if (rc) return die("ItrReader", rc);
        std::vector<float> base((size_t)N * D);
        rc = dpq_read_vecs_range(base_path.c_str(), bvecs, 0, N, &D, base.data());
        if (rc) return die("ItrReader", rc);
        std::vector<uint32_t> vec_id((size_t)N);
        const std::string nodes_path = dataset + "/M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) +
                                       "_Approx_TreeNodesDFS_N" + std::to_string(N);
        rc = dpq_read_qnode_ids(nodes_path.c_str(), N, vec_id.data());
        if (rc) return die("read TreeNodesDFS", rc);
        if (dpq_device_count() < 1) {
            std::cout << "no GPU visible: this build has no CPU path" << std::endl;
            return 1;
        }
        char fname[4096];
        rc = dpq_dtc_file_name(dataset.c_str(), PQ_M, PQ_K, N, fname, sizeof fname);
        if (rc) return die("file name", rc);
        dpq_index* idx = nullptr;
        dpq_open_opts o;
        memset(&o, 0, sizeof o);
        rc = dpq_open_file(fname, PQ_M, PQ_K, &o, &idx);
        if (rc) return die("dpq_open_file", rc);
        rc = dpq_set_codebook(idx, codewords.data(), cDs);
        if (rc) return die("dpq_set_codebook", rc);
        dpq_refine_opts ro;
        memset(&ro, 0, sizeof ro);
        ro.M2 = refine_m2;
        ro.K2 = refine_k2;
        ro.train_n = train_size;
        ro.seed = seed;
        dpq_refine* lvl = nullptr;
        const double t0 = Elapsed();
        rc = dpq_refine_build(idx, base.data(), N, D, vec_id.data(), &ro, &lvl);
        if (rc) return die("dpq_refine_build", rc);
        const double elapsed = Elapsed() - t0;
        int32_t M2 = 0, K2 = 0, Ds2 = 0;
        int64_t n_local = 0;
        rc = dpq_refine_get(lvl, &M2, &K2, &Ds2, &n_local, nullptr, nullptr);
        if (rc) return die("dpq_refine_get", rc);
        std::vector<float> cw2((size_t)M2 * K2 * Ds2);
        std::vector<uint8_t> codes2((size_t)n_local * M2);
        rc = dpq_refine_get(lvl, nullptr, nullptr, nullptr, nullptr, cw2.data(), codes2.data());
        if (rc) return die("dpq_refine_get", rc);
        dpq_refine_free(lvl);
        dpq_close(idx);
        const std::string tag = "M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K);
        const std::string tag2 = "M" + std::to_string(M2) + "K" + std::to_string(K2);
        const std::string cw2_path = dataset + "/" + tag + "_refine_" + tag2 + "codewords.txt";
        const std::string codes2_path = dataset + "/codes.bin.refine." + tag + tag2 + "N" + std::to_string(N);
        rc = dpq_write_codewords(cw2_path.c_str(), cw2.data(), M2, K2, Ds2);
        if (rc) return die("PQ::WriteCodewords", rc);
        rc = dpq_write_codes_plain(codes2_path.c_str(), codes2.data(), n_local, M2);
        if (rc) return die("PQTree::Write", rc);
        std::cout << "refine level M2 = " << M2 << " K2 = " << K2 << " Ds2 = " << Ds2 << " over " << n_local << " nodes in "
                  << elapsed << " [sec] -> " << cw2_path << ", " << codes2_path << std::endl;
        return 0;
    }
    if (task == "recall") {
        // The other binary's `pqtree -task recall` (main.cpp:727-803) over this engine's answer: DTC query, DFS
        // positions -> vector ids (QNode.vec_id), against groundtruth/N{N}Top{G}.txt; -rerank R re-scores the PQ top-R
        // against base.{ext} (main.cpp:898-939) and reports the recall of that answer too.
        if (PQ_M <= 0 || PQ_K <= 0 || dataset.empty() || N < 1 || !topk_given || top_k < 1 || query_size < 1) {
            std::cout << "usage: deltapq -dataset DIR -task recall -m M -k K -N N -query_size Q -topk K [-gt_topk G] [-rerank R]"
                         " [-store f16|bf16|sq8|sq4] [-ext fvecs|bvecs] [-filter FILE] [-opq] [-refine R [-m2 M2] [-k2 K2]] [-metric l2|ip] [-ivf CENTROIDS.fvecs -nprobe P]   (-refine: the"
                         " level of -task refine, M <= 8; -metric ip: dpq_query_batch_ip against the .ip.txt truth, not with -refine;"
                         " -ivf: the lists' recall beside the exhaustive line under the same -filter and -metric, not with -refine, -opq or -gpus above 1;"
                         " -store: the re-rank once more from the base narrowed to fp16 / bf16, or scalar-quantised to 8 / 4 bits)" << std::endl;
            return 2;
        }
        if (gt_topk < 0) gt_topk = top_k;
        if (gt_topk < top_k) {
            std::cout << "-gt_topk " << gt_topk << " is below -topk " << top_k << std::endl;
            return 1;
        }
        if (rerank != 0 && (rerank < top_k || rerank > 2048)) {
            std::cout << "-rerank " << rerank << " outside " << top_k << "..2048" << std::endl;
            return 1;
        }
        // -filter FILE: dpq_query_batch_filtered under the bitmap translated to DFS positions, against the .filtered.txt truth
        const bool filtered = !filter_path.empty();
        if (filtered && rerank) {
            std::cout << "-rerank cannot be combined with -filter: there is no filtered re-rank" << std::endl;
            return 1;
        }
        if (refine_r != 0 && (refine_r < top_k || refine_r > 2048 || filtered || PQ_M > 8)) {
            std::cout << "-refine " << refine_r << " outside " << top_k << "..2048, or combined with -filter, or M > 8" << std::endl;
            return 1;
        }
        // -ivf CENTROIDS.fvecs -nprobe P: inverted lists built from the centroids file over the opened index
        // (dpq_ivf_build); the recall of dpq_ivf_search is printed beside the exhaustive line, against the same truth file.
        // With -filter FILE the lists are searched under the same filter (dpq_ivf_search_filtered), with -metric ip by
        // inner product, coarse step included (dpq_ivf_search_ip, which takes the filter too)
        const bool with_ivf = !ivf_path.empty();
        if (with_ivf && (refine_r != 0 || gpus > 1 || opq || nprobe < 1 || nprobe > 1024 || top_k > 2048)) {
            std::cout << "-ivf FILE -nprobe P (1..1024, -topk up to 2048) cannot be combined with -refine, -opq "
                         "(the centroids would have to be in the rotated space) or -gpus above 1" << std::endl;
            return 1;
        }
        const bool bvecs = ext == "bvecs";
        const std::string cw_path = dataset + "/M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) + "codewords.txt";
        int32_t cM = 0, cK = 0, cDs = 0;
        int rc = dpq_read_codewords(cw_path.c_str(), &cM, &cK, &cDs, nullptr);
        if (rc) return die("ReadCodewords", rc);
        std::vector<float> codewords((size_t)cM * cK * cDs);
        rc = dpq_read_codewords(cw_path.c_str(), &cM, &cK, &cDs, codewords.data());
        if (rc) return die("ReadCodewords", rc);
        if (cM != PQ_M || cK != PQ_K) {
            std::cout << "codewords file is M=" << cM << " K=" << cK << std::endl;
            return 1;
        }
        const std::string q_path = dataset + "/query." + ext;
        int64_t nq_file = 0;
        int32_t D = 0;
        rc = dpq_read_vecs(q_path.c_str(), bvecs, &nq_file, &D, nullptr, 0);
        if (rc) return die("ReadTopN", rc);
        if (query_size > nq_file) {
            std::cout << "-query_size " << query_size << " exceeds the " << nq_file << " available queries" << std::endl;
            return 1;
        }
        const int nq = query_size;
        std::vector<float> queries((size_t)nq * D);
        rc = dpq_read_vecs(q_path.c_str(), bvecs, &nq_file, &D, queries.data(), nq);
        if (rc) return die("ReadTopN", rc);
        if (D != PQ_M * cDs) {
            std::cout << "query dimension " << D << " != M*Ds = " << PQ_M * cDs << std::endl;
            return 1;
        }
        std::vector<float> ivf_centroids;
        int64_t nlist = 0;
        if (with_ivf) {
            int32_t Dc = 0;
            rc = dpq_read_vecs(ivf_path.c_str(), 0, &nlist, &Dc, nullptr, 0);
            if (rc) return die("read -ivf centroids", rc);
            if (Dc != D || nlist < 1 || nlist > 65536 || nprobe > nlist) {
                std::cout << ivf_path << " holds " << nlist << " x " << Dc << ": needs 1..65536 centroids of dimension " << D
                          << " and -nprobe " << nprobe << " at most their number" << std::endl;
                return 1;
            }
            ivf_centroids.resize((size_t)nlist * Dc);
            rc = dpq_read_vecs(ivf_path.c_str(), 0, &nlist, &Dc, ivf_centroids.data(), nlist);
            if (rc) return die("read -ivf centroids", rc);
        }
        // -opq: the PQ query sees rotated queries; ground truth and the exact re-rank keep the raw ones
        std::vector<float> pq_queries_store;
        if (opq) {
            pq_queries_store = queries;
            if (rotate_rows(dataset, PQ_M, PQ_K, &pq_queries_store, nq, D)) return 1;
        }
        const std::vector<float>& pq_queries = opq ? pq_queries_store : queries;
        const std::string gt_path = dataset + "/groundtruth/N" + std::to_string(N) + "Top" + std::to_string(gt_topk) +
                                    (ip ? ".ip" : "") + (filtered ? ".filtered.txt" : ".txt");
        int32_t g_nq = 0, g_k = 0;
        rc = dpq_read_groundtruth(gt_path.c_str(), &g_nq, &g_k, nullptr, nullptr);
        if (rc) return die("read_groundtruth", rc);
        if (g_nq < nq || g_k < top_k) {
            std::cout << gt_path << " holds " << g_nq << " x " << g_k << ", needed " << nq << " x " << top_k << std::endl;
            return 1;
        }
        std::vector<int32_t> truth((size_t)g_nq * g_k);
        std::vector<float> truth_d((size_t)g_nq * g_k);
        rc = dpq_read_groundtruth(gt_path.c_str(), &g_nq, &g_k, truth.data(), truth_d.data());
        if (rc) return die("read_groundtruth", rc);
        std::vector<uint32_t> vec_id((size_t)N);
        const std::string nodes_path = dataset + "/M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) +
                                       "_Approx_TreeNodesDFS_N" + std::to_string(N);
        rc = dpq_read_qnode_ids(nodes_path.c_str(), N, vec_id.data());
        if (rc) return die("read TreeNodesDFS", rc);
        if (dpq_device_count() < 1) {
            std::cout << "no GPU visible: this build has no CPU query path" << std::endl;
            return 1;
        }
        char fname[4096];
        rc = dpq_dtc_file_name(dataset.c_str(), PQ_M, PQ_K, N, fname, sizeof fname);
        if (rc) return die("file name", rc);
        dpq_index* idx = nullptr;
        dpq_open_opts o;
        memset(&o, 0, sizeof o);
        rc = dpq_open_file(fname, PQ_M, PQ_K, &o, &idx);
        if (rc) return die("dpq_open_file", rc);
        rc = dpq_set_codebook(idx, codewords.data(), cDs);
        if (rc) return die("dpq_set_codebook", rc);
        const int R = rerank ? rerank : top_k;
        std::vector<int32_t> pos((size_t)nq * R), found((size_t)nq * R);
        std::vector<float> pq_d((size_t)nq * R);
        dpq_filter* filt = nullptr;
        if (filtered) {
            std::vector<uint32_t> f_words, dfs_words((size_t)((N + 1 + 31) / 32));
            int64_t f_bits = 0;
            rc = read_filter(filter_path, &f_words, &f_bits);
            if (rc) return die("dpq_read_bitmap", rc);
            rc = dpq_bitmap_to_dfs(f_words.data(), f_bits, vec_id.data(), N, dfs_words.data());
            if (rc) return die("dpq_bitmap_to_dfs", rc);
            rc = dpq_filter_create(idx, dfs_words.data(), N + 1, &filt);
            if (rc) return die("dpq_filter_create", rc);
        }
        const double t0 = Elapsed();
        for (int q0 = 0; q0 < nq; q0 += 1024) {
            const int m = std::min(1024, nq - q0);
            const float* qp = pq_queries.data() + (size_t)q0 * D;
            int32_t* ids_at = pos.data() + (size_t)q0 * R;
            float* d_at = pq_d.data() + (size_t)q0 * R;
            rc = ip         ? dpq_query_batch_ip(idx, filt, qp, m, R, ids_at, d_at, nullptr, nullptr)  // filt may be NULL
                 : filtered ? dpq_query_batch_filtered(idx, filt, qp, m, R, ids_at, d_at)
                            : dpq_query_batch(idx, qp, m, R, ids_at, d_at);
            if (rc) return die(ip ? "dpq_query_batch_ip" : filtered ? "dpq_query_batch_filtered" : "dpq_query_batch", rc);
        }
        std::cout << (Elapsed() - t0) / (double)nq * 1000 << " [msec/query] " << std::endl;
        std::vector<int32_t> ref_pos;
        if (refine_r) {  // the level -task refine wrote: the PQ top-R refined to top_k on the device
            const int M2 = refine_m2 ? refine_m2 : PQ_M, K2 = refine_k2 ? refine_k2 : 256;
            const std::string tag = "M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K);
            const std::string tag2 = "M" + std::to_string(M2) + "K" + std::to_string(K2);
            const std::string cw2_path = dataset + "/" + tag + "_refine_" + tag2 + "codewords.txt";
            const std::string codes2_path = dataset + "/codes.bin.refine." + tag + tag2 + "N" + std::to_string(N);
            int32_t rM = 0, rK = 0, rDs = 0;
            rc = dpq_read_codewords(cw2_path.c_str(), &rM, &rK, &rDs, nullptr);
            if (rc) return die("ReadCodewords (refine)", rc);
            std::vector<float> cw2((size_t)rM * rK * rDs);
            rc = dpq_read_codewords(cw2_path.c_str(), &rM, &rK, &rDs, cw2.data());
            if (rc) return die("ReadCodewords (refine)", rc);
            int64_t n2 = 0;
            rc = dpq_read_codes_plain(codes2_path.c_str(), rM, &n2, nullptr);
            if (rc) return die("PQTree::Read (refine)", rc);
            std::vector<uint8_t> codes2((size_t)n2 * rM);
            rc = dpq_read_codes_plain(codes2_path.c_str(), rM, &n2, codes2.data());
            if (rc) return die("PQTree::Read (refine)", rc);
            dpq_refine* lvl = nullptr;
            rc = dpq_refine_create(idx, cw2.data(), rM, rK, rDs, codes2.data(), n2, &lvl);
            if (rc) return die("dpq_refine_create", rc);
            ref_pos.resize((size_t)nq * top_k);
            std::vector<float> ref_d((size_t)nq * top_k);
            const double t1 = Elapsed();
            rc = dpq_query_batch_refined(idx, lvl, nullptr, queries.data(), nq, refine_r, top_k, ref_pos.data(), ref_d.data());
            if (rc) return die("dpq_query_batch_refined", rc);
            std::cout << "refined query " << (Elapsed() - t1) / (double)nq * 1000 << " [msec/query] " << std::endl;
            dpq_refine_free(lvl);
        }
        std::vector<int32_t> ivf_pos;
        if (with_ivf) {
            dpq_ivf* ivf = nullptr;
            const double t1 = Elapsed();
            rc = dpq_ivf_build(idx, ivf_centroids.data(), (int)nlist, &ivf);
            if (rc) return die("dpq_ivf_build", rc);
            dpq_ivf_stats st;
            rc = dpq_ivf_get_info(ivf, &st);
            if (rc) return die("dpq_ivf_get_info", rc);
            std::cout << "ivf: " << st.nlist << " lists over " << st.n_assigned << " codes, longest " << st.max_list_len << ", "
                      << st.device_bytes << " bytes, built in " << (Elapsed() - t1) * 1000 << " [msec]" << std::endl;
            ivf_pos.resize((size_t)nq * top_k);
            std::vector<float> ivf_d((size_t)nq * top_k);
            const double t2 = Elapsed();
            rc = ip         ? dpq_ivf_search_ip(ivf, filt, pq_queries.data(), nq, nprobe, top_k, ivf_pos.data(), ivf_d.data(), nullptr,
                                                nullptr)  // filt may be NULL
                 : filtered ? dpq_ivf_search_filtered(ivf, filt, pq_queries.data(), nq, nprobe, top_k, ivf_pos.data(), ivf_d.data())
                            : dpq_ivf_search(ivf, pq_queries.data(), nq, nprobe, top_k, ivf_pos.data(), ivf_d.data());
            if (rc) return die(ip ? "dpq_ivf_search_ip" : filtered ? "dpq_ivf_search_filtered" : "dpq_ivf_search", rc);
            std::cout << "ivf query " << (Elapsed() - t2) / (double)nq * 1000 << " [msec/query] " << std::endl;
            dpq_ivf_free(ivf);
        }
        dpq_filter_free(filt);
        dpq_close(idx);
        for (size_t i = 0; i < found.size(); ++i) {
            int64_t p = pos[i];
            if (p == N && N % 2 == 0) p = N - 1;  // the even-N id of the last DFS node (h:2949, 2970)
            found[i] = p < 0 || p >= N ? -1 : (int32_t)vec_id[(size_t)p];
        }
        double rec = 0;
        rc = dpq_recall(found.data(), R, top_k, truth.data(), g_k, top_k, nq, &rec);
        if (rc) return die("dpq_recall", rc);
        char line[128];
        snprintf(line, sizeof line, filtered ? "filtered recall@%d = %.6f" : "recall@%d = %.6f", top_k, rec);
        std::cout << line << std::endl;
        if (with_ivf) {
            std::vector<int32_t> ivf_found(ivf_pos.size());
            for (size_t i = 0; i < ivf_found.size(); ++i) {
                int64_t p = ivf_pos[i];
                if (p == N && N % 2 == 0) p = N - 1;
                ivf_found[i] = p < 0 || p >= N ? -1 : (int32_t)vec_id[(size_t)p];
            }
            double ivf_rec = 0;
            rc = dpq_recall(ivf_found.data(), top_k, top_k, truth.data(), g_k, top_k, nq, &ivf_rec);
            if (rc) return die("dpq_recall", rc);
            snprintf(line, sizeof line, "ivf recall@%d = %.6f (nlist %d, nprobe %d)", top_k, ivf_rec, (int)nlist, nprobe);
            std::cout << line << std::endl;
        }
        if (refine_r) {
            std::vector<int32_t> ref_found(ref_pos.size());
            for (size_t i = 0; i < ref_found.size(); ++i) {
                int64_t p = ref_pos[i];
                if (p == N && N % 2 == 0) p = N - 1;
                ref_found[i] = p < 0 || p >= N ? -1 : (int32_t)vec_id[(size_t)p];
            }
            double ref_rec = 0;
            rc = dpq_recall(ref_found.data(), top_k, top_k, truth.data(), g_k, top_k, nq, &ref_rec);
            if (rc) return die("dpq_recall", rc);
            snprintf(line, sizeof line, "refine: recall@%d PQ %.6f -> top-%d refined %.6f", top_k, rec, refine_r, ref_rec);
            std::cout << line << std::endl;
        }
        if (rerank) {
            const std::string base_path = dataset + "/base." + ext;
            int32_t Db = 0;
            rc = dpq_read_vecs_range(base_path.c_str(), bvecs, 0, N, &Db, nullptr);
            if (!rc && Db != D) {
                std::cout << "query dimension " << D << " != base dimension " << Db << std::endl;
                return 1;
            }
            if (rc) return die("ItrReader", rc);
            dpq_flat* f = nullptr;
            std::vector<uint8_t> queries8;
            if (bvecs) {  // bytes stay bytes: a byte handle and the _u8 / _ip_u8 calls, the same bits
                std::vector<uint8_t> base8((size_t)N * D);
                queries8.resize((size_t)nq * D);
                rc = dpq_read_bvecs_range(base_path.c_str(), 0, N, &Db, base8.data());
                if (!rc) rc = dpq_read_bvecs_range(q_path.c_str(), 0, nq, &Db, queries8.data());
                if (rc) return die("ItrReader", rc);
                rc = dpq_flat_open_u8(base8.data(), N, D, 0, 0, &f);
            } else {
                std::vector<float> base((size_t)N * D);
                rc = dpq_read_vecs_range(base_path.c_str(), bvecs, 0, N, &Db, base.data());
                if (rc) return die("ItrReader", rc);
                rc = dpq_flat_open(base.data(), N, D, 0, 0, &f);
            }
            if (rc == DPQ_ERR_NOMEM) {
                std::cout << "-rerank: base." << ext << " (" << N << " x " << D << ") does not fit into device memory" << std::endl;
                return 1;
            }
            if (rc) return die(bvecs ? "dpq_flat_open_u8" : "dpq_flat_open", rc);
            rc = dpq_flat_set_id_map(f, vec_id.data(), N);
            if (rc) return die("dpq_flat_set_id_map", rc);
            std::vector<int32_t> r_ids((size_t)nq * top_k);
            std::vector<float> r_d((size_t)nq * top_k);
            const double t1 = Elapsed();
            rc = bvecs ? (ip ? dpq_flat_rerank_ip_u8(f, queries8.data(), nq, pos.data(), R, top_k, r_ids.data(), r_d.data())
                             : dpq_flat_rerank_u8(f, queries8.data(), nq, pos.data(), R, top_k, r_ids.data(), r_d.data()))
                 : ip  ? dpq_flat_rerank_ip(f, queries.data(), nq, pos.data(), R, top_k, r_ids.data(), r_d.data())
                       : dpq_flat_rerank(f, queries.data(), nq, pos.data(), R, top_k, r_ids.data(), r_d.data());
            if (rc)
                return die(bvecs ? (ip ? "dpq_flat_rerank_ip_u8" : "dpq_flat_rerank_u8") : ip ? "dpq_flat_rerank_ip" : "dpq_flat_rerank", rc);
            std::cout << "re-rank " << (Elapsed() - t1) / (double)nq * 1000 << " [msec/query] " << std::endl;
            dpq_flat_close(f);
            rc = dpq_recall(r_ids.data(), top_k, top_k, truth.data(), g_k, top_k, nq, &rec);
            if (rc) return die("dpq_recall", rc);
            snprintf(line, sizeof line, "reranked recall@%d = %.6f", top_k, rec);
            std::cout << line << std::endl;
            if (!store.empty()) {  // the same re-rank from the base narrowed or quantised; the truth stays fp32
                std::vector<float> base((size_t)N * D);
                rc = dpq_read_vecs_range(base_path.c_str(), bvecs, 0, N, &Db, base.data());
                if (rc) return die("ItrReader", rc);
                const float* q32 = queries.data();  // fp32, a .bvecs file widened
                if (store_sq)
                    rc = dpq_flat_open_quantised(base.data(), N, D, store == "sq8" ? DPQ_SQ_8BIT : DPQ_SQ_4BIT, nullptr, nullptr, 0, 0, &f);
                else
                    rc = dpq_flat_open_narrowed(base.data(), N, D, store == "f16" ? DPQ_HALF_F16 : DPQ_HALF_BF16, 0, 0, &f);
                if (rc) return die(store_sq ? "dpq_flat_open_quantised" : "dpq_flat_open_narrowed", rc);
                rc = dpq_flat_set_id_map(f, vec_id.data(), N);
                if (rc) return die("dpq_flat_set_id_map", rc);
                const double t2 = Elapsed();
                rc = ip ? dpq_flat_rerank_ip(f, q32, nq, pos.data(), R, top_k, r_ids.data(), r_d.data())
                        : dpq_flat_rerank(f, q32, nq, pos.data(), R, top_k, r_ids.data(), r_d.data());
                if (rc) return die(ip ? "dpq_flat_rerank_ip" : "dpq_flat_rerank", rc);
                std::cout << "re-rank (" << store << " store) " << (Elapsed() - t2) / (double)nq * 1000 << " [msec/query] " << std::endl;
                dpq_flat_close(f);
                rc = dpq_recall(r_ids.data(), top_k, top_k, truth.data(), g_k, top_k, nq, &rec);
                if (rc) return die("dpq_recall", rc);
                snprintf(line, sizeof line, "reranked recall@%d (%s store) = %.6f", top_k, store.c_str(), rec);
                std::cout << line << std::endl;
            }
        }
        return 0;
    }
    const bool pqscan = task == "pqscan";  // main:496-556: uncompressed comparator over codes.bin.plain
    // -task batch_query (main:351-420) is accepted as an alias of -task query: the engine behind `query`
    // already decodes every chunk once for a whole batch of queries, with the -task query arithmetic and ids
    // (the reference's batch variant accumulates in fp32 and records the second node of a pair under the
    // first one's id, h:3079, h:3389-3392 -- not reproduced).
    if (task == "batch_query") {
        std::cout << "NOTE: -task batch_query runs as -task query here (its arithmetic, ids and tie order); the reference's "
                     "batch variant (fp32 accumulation, pair ids: h:3079, h:3389-3392) is a documented deviation, not reproduced"
                  << std::endl;
        task = "query";
    }
    if (task != "query" && task != "query_im" && !pqscan) {
        std::cout << "deltapq (MI355X build): -task query, query_im, pqscan, approx_tree, encode, learn, ivf_learn, decompress, groundtruth and recall are implemented (batch_query = "
                     "alias of query); got '" << task
                  << "'" << std::endl;
        return 2;
    }
    if (PQ_M <= 0 || PQ_K <= 0 || dataset.empty()) {
        std::cout << "usage: deltapq -dataset DIR -task query -m M -k K -N N -query_size Q -topk K [-ext fvecs|bvecs]"
                     " [-debug] [-gpus G] [-out FILE] [-opq]" << std::endl;
        return 2;
    }

    // main:274-275
    const std::string cw_path = dataset + "/M" + std::to_string(PQ_M) + "K" + std::to_string(PQ_K) + "codewords.txt";
    std::cout << cw_path << std::endl;
    int32_t cM = 0, cK = 0, cDs = 0;
    int rc = dpq_read_codewords(cw_path.c_str(), &cM, &cK, &cDs, nullptr);
    if (rc) return die("ReadCodewords", rc);
    std::vector<float> codewords((size_t)cM * cK * cDs);
    rc = dpq_read_codewords(cw_path.c_str(), &cM, &cK, &cDs, codewords.data());
    if (rc) return die("ReadCodewords", rc);
    std::cout << "++++++ codewords read from +++++" << cw_path << std::endl;
    std::cout << "++++++ " << cM << "Ks " << cK << "Ds " << cDs << std::endl;
    if (cM != PQ_M || cK != PQ_K) {
        std::cout << "codewords file is M=" << cM << " K=" << cK << " but -m " << PQ_M << " -k " << PQ_K << std::endl;
        return 1;
    }

    // index file (h:2812-2814), or the plain code file for pqscan (h:2616-2618); like the
    // reference the caller must pass -N (it is part of the file name)
    char fname[4096];
    int64_t n_codes = 0, n_bytes = 0;
    if (pqscan) {
        // the reference's pqscan opens codes.bin.plain.M{M}K{K} (h:2616-2617); the encoder and approx_tree
        // use the name with the N{N} suffix (main:76-77) -- accept either
        snprintf(fname, sizeof fname, "%s/codes.bin.plain.M%dK%d", dataset.c_str(), PQ_M, PQ_K);
        rc = dpq_read_codes_plain(fname, PQ_M, &n_codes, nullptr);
        if (rc) {
            snprintf(fname, sizeof fname, "%s/codes.bin.plain.M%dK%dN%lld", dataset.c_str(), PQ_M, PQ_K, N);
            rc = dpq_read_codes_plain(fname, PQ_M, &n_codes, nullptr);
        }
        std::cout << fname << std::endl;
        if (rc) return die("open codes", rc);
        std::cout << "top_k = " << top_k << std::endl;  // main:504
    } else {
        rc = dpq_dtc_file_name(dataset.c_str(), PQ_M, PQ_K, N, fname, sizeof fname);
        if (rc) return die("file name", rc);
        std::cout << fname << std::endl;
        rc = dpq_read_dtc_header(fname, &n_codes, &n_bytes);
        if (rc) return die("open index", rc);
    }
    if (N == -1) N = n_codes;  // h:2825
    if (N < 1 || N > n_codes) {
        std::cout << "-N " << N << " outside 1.." << n_codes << std::endl;
        return 1;
    }
    if (N != n_codes)  // h:2826-2829 / main:629-632: the first N codes of a larger index
        std::cout << "scan only part of the codes " << N << " / " << n_codes << std::endl;
    std::cout << "M = " << PQ_M << std::endl;
    std::cout << "K = " << PQ_K << std::endl;
    std::cout << "N = " << N << std::endl;
    std::cout << dataset << std::endl;

    // main:303-308
    const std::string q_path = dataset + "/query." + ext;
    std::cout << "In ReadTopN " << q_path << std::endl;
    int64_t nq_file = 0;
    int32_t D = 0;
    rc = dpq_read_vecs(q_path.c_str(), ext == "bvecs", &nq_file, &D, nullptr, 0);
    if (rc) return die("ReadTopN", rc);
    std::cout << nq_file << " query vectors read from " << q_path << std::endl;
    int64_t nq = nq_file;
    if (nq > 10000) nq = 10000;
    if (query_size != -1) {
        if (query_size > nq) {
            std::cout << "-query_size " << query_size << " exceeds the " << nq << " available queries" << std::endl;
            return 1;
        }
        nq = query_size;
    }
    std::vector<float> queries((size_t)nq * D);
    rc = dpq_read_vecs(q_path.c_str(), ext == "bvecs", &nq_file, &D, queries.data(), nq);
    if (rc) return die("ReadTopN", rc);
    if (D != PQ_M * cDs) {
        std::cout << "query dimension " << D << " != M*Ds = " << PQ_M * cDs << std::endl;
        return 1;
    }

    const int ndev = dpq_device_count();
    if (ndev < 1) {
        std::cout << "no GPU visible: this build has no CPU query path" << std::endl;
        return 1;
    }
    if (opq && rotate_rows(dataset, PQ_M, PQ_K, &queries, nq, D)) return 1;  // the index holds codes of rotated vectors
    if (gpus < 1) gpus = 1;
    if (gpus > ndev) {
        std::cout << "-gpus " << gpus << " but only " << ndev << " device(s) visible" << std::endl;
        return 1;
    }

    // load once: parse + transcode + upload, one shard per GPU
    std::vector<dpq_index*> shards((size_t)gpus, nullptr);
    const double tl0 = Elapsed();
    for (int g = 0; g < gpus; ++g) {
        dpq_open_opts o;
        memset(&o, 0, sizeof o);
        o.device = g;
        o.shard_rank = g;
        o.shard_count = gpus;
        o.num_codes = N != n_codes ? (int32_t)N : 0;
        rc = pqscan ? dpq_open_plain_file(fname, PQ_M, PQ_K, &o, &shards[(size_t)g])
                    : dpq_open_file(fname, PQ_M, PQ_K, &o, &shards[(size_t)g]);
        if (rc) return die("dpq_open_file", rc);
        rc = dpq_set_codebook(shards[(size_t)g], codewords.data(), cDs);
        if (rc) return die("dpq_set_codebook", rc);
    }
    std::cout << "index resident on " << gpus << " GPU(s) in " << (Elapsed() - tl0) << " [sec]" << std::endl;

    // ranked_scores[q] = vector<pair<int,float>>(top_k)  (main:310-311), flattened
    std::vector<int32_t> ids((size_t)nq * top_k);
    std::vector<float> dists((size_t)nq * top_k);
    std::vector<int32_t> part_ids;
    std::vector<float> part_dists;
    if (gpus > 1) {
        part_ids.resize((size_t)gpus * nq * top_k);
        part_dists.resize((size_t)gpus * nq * top_k);
    }

    const double t0 = Elapsed();  // main:327
    if (gpus == 1) {
        // the reference's loop, one query per call (main:328-339), as batches in flight: host buffers in and out, the
        // copies of neighbouring batches beside a batch's kernels (dpq_query_batch_host_async, page-locked buffers)
        const int64_t chunk = 1024;
        const int D = PQ_M * cDs;
        dpq_pin_host(queries.data(), (int64_t)(queries.size() * sizeof(float)));   // (not fatal if refused: the copies then run unpipelined)
        dpq_pin_host(ids.data(), (int64_t)(ids.size() * sizeof(int32_t)));
        dpq_pin_host(dists.data(), (int64_t)(dists.size() * sizeof(float)));
        for (int64_t q0 = 0; q0 < nq && !rc; q0 += chunk) {
            const int n = (int)std::min<int64_t>(chunk, nq - q0);
            rc = dpq_query_batch_host_async(shards[0], queries.data() + (size_t)q0 * D, n, top_k, ids.data() + (size_t)q0 * top_k,
                                            dists.data() + (size_t)q0 * top_k);
        }
        if (rc) return die("dpq_query_batch_host_async", rc);
        rc = dpq_finish(shards[0]);
        if (rc) return die("dpq_finish", rc);
        dpq_unpin_host(queries.data());
        dpq_unpin_host(ids.data());
        dpq_unpin_host(dists.data());
    } else {
        std::vector<int> rcs((size_t)gpus, 0);
        std::vector<std::string> msgs((size_t)gpus);
        std::vector<std::thread> th;
        for (int g = 0; g < gpus; ++g)
            th.emplace_back([&, g]() {
                rcs[(size_t)g] = dpq_query_batch(shards[(size_t)g], queries.data(), (int)nq, top_k,
                                                 part_ids.data() + (size_t)g * nq * top_k,
                                                 part_dists.data() + (size_t)g * nq * top_k);
                if (rcs[(size_t)g]) msgs[(size_t)g] = dpq_last_error();
            });
        for (auto& t : th) t.join();
        for (int g = 0; g < gpus; ++g)
            if (rcs[(size_t)g]) {
                std::cout << "shard " << g << ": " << dpq_strerror(rcs[(size_t)g]) << ": " << msgs[(size_t)g]
                          << std::endl;
                return 1;
            }
        rc = dpq_merge_topk_host(part_ids.data(), part_dists.data(), gpus, (int)nq, top_k, ids.data(), dists.data());
        if (rc) return die("dpq_merge_topk_host", rc);
    }
    const double elapsed = Elapsed() - t0;
    if (debug)  // main:340-343: top-1 per query
        for (int64_t q = 0; q < nq; ++q)
            std::cout << ids[(size_t)q * top_k] << " " << dists[(size_t)q * top_k] << std::endl;
    std::cout << elapsed / (double)nq * 1000 << " [msec/query] " << std::endl;  // main:345
    std::cout << nq << " queries run" << std::endl;                              // main:347

    if (!out_path.empty()) {
        FILE* f = fopen(out_path.c_str(), "wb");
        if (!f) {
            std::cout << "cannot open " << out_path << std::endl;
            return 1;
        }
        int64_t hdr[2] = {nq, top_k};
        fwrite(hdr, sizeof(int64_t), 2, f);
        fwrite(ids.data(), sizeof(int32_t), ids.size(), f);
        fwrite(dists.data(), sizeof(float), dists.size(), f);
        fclose(f);
    }
    for (auto* s : shards) dpq_close(s);
    std::cout << "===========================" << std::endl << std::endl;  // main:711
    return 0;
}
